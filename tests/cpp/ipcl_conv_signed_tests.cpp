// C++ tests of ipcl::ext::conv2dSigned / conv1dSigned (include/ipcl/ext/conv.hpp) and ipcl::ext::sparseMatVecSigned
// (include/ipcl/ext/linear.hpp) on the GPU: the signed-weight encrypted convolution and sparse product against decrypt --
// Dec(out) in host BigNumber arithmetic --, against the route composed from two unsigned calls and a subtraction
// (ipcl::ext::subtract), and their errors.  The reference has no signed weights: its route is
// CipherText::operator*(PlainText) with w mod n (ipcl/ciphertext.cpp:83-107), a key-width exponent per term.
#include <cstdint>
#include <cstdio>
#include <functional>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "ipcl/ext/arith.hpp"
#include "ipcl/ext/conv.hpp"
#include "ipcl/ext/linear.hpp"
#include "ipcl/ipcl.hpp"

static int g_failed = 0, g_checks = 0;
#define EXPECT_TRUE(c)                                                                 \
  do {                                                                                 \
    ++g_checks;                                                                        \
    if (!(c)) { ++g_failed; std::printf("  FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); } \
  } while (0)
#define EXPECT_EQ(a, b) EXPECT_TRUE((a) == (b))
#define EXPECT_THROW(stmt)                                        \
  do {                                                            \
    bool thrown_ = false;                                         \
    try { stmt; } catch (const std::runtime_error&) { thrown_ = true; } \
    EXPECT_TRUE(thrown_);                                         \
  } while (0)

struct Case { const char* name; std::function<void()> fn; };
static std::vector<Case>& cases() { static std::vector<Case> c; return c; }
struct Reg { Reg(const char* n, std::function<void()> f) { cases().push_back({n, f}); } };
#define TEST(name) static void name(); static Reg reg_##name(#name, name); static void name()

static std::vector<uint32_t> random_u32(size_t n, uint32_t seed) {
  std::mt19937 rng(seed);
  std::vector<uint32_t> v(n);
  for (auto& x : v) x = rng();
  return v;
}
// signed weights of up to 31 bits and a sign, with the edges among them
static std::vector<int64_t> random_signed(size_t n, uint32_t seed) {
  std::mt19937 rng(seed);
  std::vector<int64_t> v(n);
  for (auto& x : v) x = (int64_t)(rng() & 0x7fffffffu) * ((rng() & 1u) ? -1 : 1);
  const int64_t edges[] = {0, -1, 1, -0x7fffffffLL, 0x7fffffffLL};
  for (size_t k = 0; k < n && k < 5; ++k) v[k] = edges[k];
  return v;
}
static void split(const std::vector<int64_t>& w, std::vector<uint32_t>* wp, std::vector<uint32_t>* wn) {
  wp->resize(w.size());
  wn->resize(w.size());
  for (size_t k = 0; k < w.size(); ++k) {
    (*wp)[k] = w[k] > 0 ? (uint32_t)w[k] : 0u;
    (*wn)[k] = w[k] < 0 ? (uint32_t)(-w[k]) : 0u;
  }
}

static ipcl::KeyPair& shared_key() {
  static ipcl::KeyPair key = ipcl::generateKeypair(2048, true);
  return key;
}

// a running signed sum modulo n
struct SignedSum {
  BigNumber pos{0u}, neg{0u};
  void add(int64_t e, uint32_t m) {
    const BigNumber term = BigNumber((uint32_t)(e < 0 ? -e : e)) * BigNumber(m);
    if (e < 0) neg = neg + term;
    else pos = pos + term;
  }
  BigNumber mod(const BigNumber& n) const { return (pos % n + n - neg % n) % n; }
};

// the cross-correlation of the plaintext images with the signed filters, mod n
static std::vector<BigNumber> host_conv(const std::vector<uint32_t>& m, const std::vector<int64_t>& w, const ipcl::ext::Conv2dShape& s,
                                        const BigNumber& n) {
  std::vector<BigNumber> out;
  const size_t oh = s.outHeight(), ow = s.outWidth();
  for (size_t im = 0; im < s.n_img; ++im)
    for (size_t co = 0; co < s.c_out; ++co)
      for (size_t oy = 0; oy < oh; ++oy)
        for (size_t ox = 0; ox < ow; ++ox) {
          SignedSum acc;
          for (size_t ci = 0; ci < s.c_in; ++ci)
            for (size_t ky = 0; ky < s.kh; ++ky)
              for (size_t kx = 0; kx < s.kw; ++kx) {
                const long iy = (long)(oy * s.stride_h + ky) - (long)s.pad_h, ix = (long)(ox * s.stride_w + kx) - (long)s.pad_w;
                if (iy < 0 || iy >= (long)s.h || ix < 0 || ix >= (long)s.w) continue;
                acc.add(w[((co * s.c_in + ci) * s.kh + ky) * s.kw + kx], m[((im * s.c_in + ci) * s.h + (size_t)iy) * s.w + (size_t)ix]);
              }
          out.push_back(acc.mod(n));
        }
  return out;
}

TEST(conv2d_signed_against_decrypt_and_the_composed_route) {
  ipcl::KeyPair& key = shared_key();
  ipcl::ext::Conv2dShape s;
  s.n_img = 2; s.c_in = 2; s.h = 5; s.w = 4; s.c_out = 3; s.kh = 3; s.kw = 2; s.stride_h = 2; s.pad_h = 1; s.pad_w = 1;
  std::vector<uint32_t> m = random_u32(s.n_img * s.c_in * s.h * s.w, 11);
  std::vector<int64_t> w = random_signed(s.c_out * s.c_in * s.kh * s.kw, 12);
  for (size_t k = 0; k < s.c_in * s.kh * s.kw; ++k) w[2 * s.c_in * s.kh * s.kw + k] = 0;     // an all-zero filter: the ciphertext 1
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  ipcl::CipherText y = ipcl::ext::conv2dSigned(w, ct, s);
  const size_t oo = s.outHeight() * s.outWidth();
  EXPECT_TRUE(y.isDeviceResident());
  EXPECT_EQ(y.getSize(), s.n_img * s.c_out * oo);
  EXPECT_EQ(y.getElement(2 * oo), BigNumber(1u));
  const std::vector<BigNumber> want = host_conv(m, w, s, *key.pub_key.getN());
  ipcl::PlainText d = key.priv_key.decrypt(y);
  for (size_t i = 0; i < want.size(); ++i) EXPECT_EQ(d.getElement(i), want[i]);
  // subtract(conv2d(w+, x), conv2d(w-, x)), bit for bit
  std::vector<uint32_t> wp, wn;
  split(w, &wp, &wn);
  ipcl::CipherText z = ipcl::ext::subtract(ipcl::ext::conv2d(ipcl::PlainText(wp), ct, s), ipcl::ext::conv2d(ipcl::PlainText(wn), ct, s));
  for (size_t i = 0; i < want.size(); ++i) EXPECT_EQ(y.getElement(i), z.getElement(i));
  // a host-constructed CipherText goes the same way; a second signed layer takes the result as it is
  ipcl::CipherText host(key.pub_key, ct.getTexts());
  ipcl::CipherText yh = ipcl::ext::conv2dSigned(w, host, s);
  for (size_t i = 0; i < want.size(); ++i) EXPECT_EQ(yh.getElement(i), y.getElement(i));
  ipcl::ext::Conv2dShape s2;
  s2.n_img = s.n_img; s2.c_in = s.c_out; s2.h = s.outHeight(); s2.w = s.outWidth(); s2.c_out = 1;
  std::vector<int64_t> w2 = {-1, 1, -2};                                                     // a 1x1 filter over the three channels
  ipcl::PlainText d2 = key.priv_key.decrypt(ipcl::ext::conv2dSigned(w2, y, s2));
  const BigNumber n = *key.pub_key.getN();
  for (size_t im = 0; im < s.n_img; ++im)
    for (size_t o = 0; o < oo; ++o) {
      const BigNumber a = want[(im * 3 + 0) * oo + o], b = want[(im * 3 + 1) * oo + o], c = want[(im * 3 + 2) * oo + o];
      EXPECT_EQ(d2.getElement(im * oo + o), (b + n - a + n - c + n - c) % n);
    }
}

TEST(conv1d_signed_is_the_one_row_case) {
  ipcl::KeyPair& key = shared_key();
  const size_t n_seq = 2, c_in = 2, len = 9, c_out = 2, k = 3;
  std::vector<uint32_t> m = random_u32(n_seq * c_in * len, 21);
  std::vector<int64_t> w = random_signed(c_out * c_in * k, 22);
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  ipcl::CipherText y = ipcl::ext::conv1dSigned(w, ct, n_seq, c_in, len, c_out, k, 2, 1);
  ipcl::ext::Conv2dShape s;
  s.n_img = n_seq; s.c_in = c_in; s.w = len; s.c_out = c_out; s.kw = k; s.stride_w = 2; s.pad_w = 1;
  EXPECT_EQ(y.getSize(), n_seq * c_out * s.outWidth());
  const std::vector<BigNumber> want = host_conv(m, w, s, *key.pub_key.getN());
  ipcl::PlainText d = key.priv_key.decrypt(y);
  for (size_t i = 0; i < want.size(); ++i) EXPECT_EQ(d.getElement(i), want[i]);
  // wide weights: the whole int64 range, against host BigNumber arithmetic: |INT64_MIN| = 2^63, INT64_MAX = 2^63 - 1
  std::vector<int64_t> wide = {INT64_MIN, INT64_MAX, -1};
  std::vector<uint32_t> mw = random_u32(5, 23);
  ipcl::CipherText one = key.pub_key.encrypt(ipcl::PlainText(mw));
  ipcl::PlainText dw = key.priv_key.decrypt(ipcl::ext::conv1dSigned(wide, one, 1, 1, 5, 1, 3));
  const BigNumber n = *key.pub_key.getN();
  const BigNumber two31(0x80000000u), two63 = two31 * two31 * BigNumber(2u);
  for (size_t i = 0; i < 3; ++i) {
    const BigNumber pos = (two63 - BigNumber(1u)) * BigNumber(mw[i + 1]);
    const BigNumber neg = two63 * BigNumber(mw[i]) + BigNumber(mw[i + 2]);
    EXPECT_EQ(dw.getElement(i), (pos % n + n - neg % n) % n);
  }
}

TEST(sparse_matvec_signed_against_decrypt_and_the_composed_route) {
  ipcl::KeyPair& key = shared_key();
  const size_t cols = 11;
  // rows of 3, 0, 20 (longer than the chunk: fold levels), 2 entries; the last row names column 4 twice with weights a and -a
  std::vector<uint64_t> row_ptr = {0, 3, 3, 23, 25};
  std::vector<uint32_t> col_idx;
  std::mt19937 rng(31);
  for (size_t t = 0; t < 23; ++t) col_idx.push_back(rng() % cols);
  col_idx.push_back(4);
  col_idx.push_back(4);
  std::vector<int64_t> w = random_signed(25, 32);
  w[23] = 123456789;
  w[24] = -123456789;
  std::vector<uint32_t> m = random_u32(cols, 33);
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  ipcl::CipherText y = ipcl::ext::sparseMatVecSigned(row_ptr, col_idx, w, ct);
  EXPECT_TRUE(y.isDeviceResident());
  EXPECT_EQ(y.getSize(), (size_t)4);
  EXPECT_EQ(y.getElement(1), BigNumber(1u));          // an empty row
  EXPECT_EQ(y.getElement(3), BigNumber(1u));          // opposite weights on one column: the ciphertext 1 exactly
  const BigNumber n = *key.pub_key.getN();
  ipcl::PlainText d = key.priv_key.decrypt(y);
  for (size_t i = 0; i < 4; ++i) {
    SignedSum acc;
    for (uint64_t t = row_ptr[i]; t < row_ptr[i + 1]; ++t) acc.add(w[t], m[col_idx[t]]);
    EXPECT_EQ(d.getElement(i), acc.mod(n));
  }
  std::vector<uint32_t> wp, wn;
  split(w, &wp, &wn);
  ipcl::CipherText z = ipcl::ext::subtract(ipcl::ext::sparseMatVec(row_ptr, col_idx, ipcl::PlainText(wp), ct),
                                           ipcl::ext::sparseMatVec(row_ptr, col_idx, ipcl::PlainText(wn), ct));
  for (size_t i = 0; i < 4; ++i) EXPECT_EQ(y.getElement(i), z.getElement(i));
  // a dense row is the signed matvec
  std::vector<uint64_t> rp = {0, cols};
  std::vector<uint32_t> all(cols);
  for (size_t j = 0; j < cols; ++j) all[j] = (uint32_t)j;
  std::vector<int64_t> wd = random_signed(cols, 34);
  EXPECT_EQ(ipcl::ext::sparseMatVecSigned(rp, all, wd, ct).getElement(0), ipcl::ext::dotSigned(wd, ct).getElement(0));
}

TEST(signed_errors) {
  ipcl::KeyPair& key = shared_key();
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(random_u32(12, 51)));
  ipcl::ext::Conv2dShape s;
  s.h = 3; s.w = 4; s.kh = 2; s.kw = 2;
  EXPECT_EQ(ipcl::ext::conv2dSigned(random_signed(4, 52), ct, s).getSize(), (size_t)6);
  EXPECT_THROW(ipcl::ext::conv2dSigned(random_signed(5, 53), ct, s));              // 5 weights for a 2x2 filter
  EXPECT_THROW(ipcl::ext::conv2dSigned(random_signed(4, 54), ipcl::CipherText(), s));   // empty CipherText
  ipcl::ext::Conv2dShape bad = s;
  bad.pad_h = 2;
  EXPECT_THROW(ipcl::ext::conv2dSigned(random_signed(4, 55), ct, bad));            // padding not smaller than the kernel
  bad = s;
  bad.stride_w = 0;
  EXPECT_THROW(ipcl::ext::conv2dSigned(random_signed(4, 56), ct, bad));
  bad = s;
  bad.h = 4;
  EXPECT_THROW(ipcl::ext::conv2dSigned(random_signed(4, 57), ct, bad));            // 12 elements are no 4 x 4 image
  EXPECT_THROW(ipcl::ext::conv1dSigned(random_signed(3, 58), ct, 1, 1, 11, 1, 3));
  std::vector<uint64_t> rp = {0, 2, 3};
  std::vector<uint32_t> ci = {0, 11, 5};
  EXPECT_EQ(ipcl::ext::sparseMatVecSigned(rp, ci, random_signed(3, 59), ct).getSize(), (size_t)2);
  EXPECT_THROW(ipcl::ext::sparseMatVecSigned(rp, ci, random_signed(2, 60), ct));   // one weight short
  EXPECT_THROW(ipcl::ext::sparseMatVecSigned({0}, {}, {}, ct));                    // no rows
  EXPECT_THROW(ipcl::ext::sparseMatVecSigned(rp, {0, 12, 5}, random_signed(3, 61), ct));   // a column index beyond the CipherText
  EXPECT_THROW(ipcl::ext::sparseMatVecSigned(rp, ci, random_signed(3, 62), ipcl::CipherText()));
  // n is no ciphertext: no inverse modulo n^2 -- an error also where no entry names its column, and the next call is served
  std::vector<BigNumber> texts = ct.getTexts();
  texts[7] = *key.pub_key.getN();
  ipcl::CipherText broken(key.pub_key, texts);
  EXPECT_THROW(ipcl::ext::sparseMatVecSigned(rp, ci, random_signed(3, 63), broken));
  EXPECT_THROW(ipcl::ext::conv2dSigned(random_signed(4, 64), broken, s));
  EXPECT_EQ(ipcl::ext::sparseMatVecSigned(rp, ci, random_signed(3, 65), ct).getSize(), (size_t)2);
  EXPECT_EQ(ipcl::ext::conv2dSigned(random_signed(4, 66), ct, s).getSize(), (size_t)6);
}

int main(int argc, char** argv) {
  ipcl::initializeContext("default");
  std::string filter = argc > 1 ? argv[1] : "";
  int ran = 0;
  for (auto& c : cases()) {
    if (!filter.empty() && std::string(c.name).find(filter) == std::string::npos) continue;
    int before = g_failed;
    std::printf("[ RUN  ] %s\n", c.name);
    try {
      c.fn();
    } catch (const std::exception& e) {
      ++g_failed;
      std::printf("  EXCEPTION: %s\n", e.what());
    }
    std::printf("[ %s ] %s\n", g_failed == before ? " OK " : "FAIL", c.name);
    ++ran;
  }
  ipcl::terminateContext();
  std::printf("%d tests, %d checks, %d failed\n", ran, g_checks, g_failed);
  return g_failed ? 1 : 0;
}
