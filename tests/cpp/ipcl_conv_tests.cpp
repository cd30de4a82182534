// C++ tests of ipcl::ext::conv2d / conv1d (include/ipcl/ext/conv.hpp), run on a real MI355X by tests/test_gpu_conv_cpp.py:
// the fused encrypted convolution against host BigNumber arithmetic (prod over the taps inside the image of
// x^w mod n^2, square and multiply), through decrypt, with a device-resident CipherText used in place and a
// host-constructed one, two layers chained, and the exceptions on a size mismatch, a shape without output, empty operands
// and negative weights.  The reference composes such a map from CipherText::operator* / operator+
// (ipcl/ciphertext.cpp:83-106, 35-72).
#include <cstdio>
#include <functional>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "ipcl/ext/conv.hpp"
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

using ipcl::ext::Conv2dShape;

static std::vector<uint32_t> random_u32(size_t n, uint32_t seed, uint32_t mask = 0xffffffffu) {
  std::mt19937 rng(seed);
  std::vector<uint32_t> v(n);
  for (auto& x : v) x = rng() & mask;
  return v;
}

static ipcl::KeyPair& shared_key() {
  static ipcl::KeyPair key = ipcl::generateKeypair(2048, true);
  return key;
}

static BigNumber pow_mod(const BigNumber& x, uint32_t e, const BigNumber& mod) {
  BigNumber acc(1u), base = x % mod;
  for (; e; e >>= 1) {
    if (e & 1u) acc = (acc * base) % mod;
    base = (base * base) % mod;
  }
  return acc;
}

static Conv2dShape shape_of(size_t n_img, size_t c_in, size_t h, size_t w, size_t c_out, size_t kh, size_t kw, size_t sh = 1,
                            size_t sw = 1, size_t ph = 0, size_t pw = 0) {
  Conv2dShape s;
  s.n_img = n_img; s.c_in = c_in; s.h = h; s.w = w; s.c_out = c_out; s.kh = kh; s.kw = kw;
  s.stride_h = sh; s.stride_w = sw; s.pad_h = ph; s.pad_w = pw;
  return s;
}

// walks the taps inside the image of every output, in output order: f(output, element of x, index into w)
template <class F>
static void for_live_taps(const Conv2dShape& s, F&& f) {
  const size_t oh = s.outHeight(), ow = s.outWidth();
  for (size_t n = 0; n < s.n_img; ++n)
    for (size_t co = 0; co < s.c_out; ++co)
      for (size_t oy = 0; oy < oh; ++oy)
        for (size_t ox = 0; ox < ow; ++ox)
          for (size_t ci = 0; ci < s.c_in; ++ci)
            for (size_t ky = 0; ky < s.kh; ++ky)
              for (size_t kx = 0; kx < s.kw; ++kx) {
                const long iy = (long)(oy * s.stride_h + ky) - (long)s.pad_h, ix = (long)(ox * s.stride_w + kx) - (long)s.pad_w;
                if (iy < 0 || iy >= (long)s.h || ix < 0 || ix >= (long)s.w) continue;
                f(((n * s.c_out + co) * oh + oy) * ow + ox, ((n * s.c_in + ci) * s.h + (size_t)iy) * s.w + (size_t)ix,
                  ((co * s.c_in + ci) * s.kh + ky) * s.kw + kx);
              }
}

static std::vector<BigNumber> host_conv(const std::vector<BigNumber>& x, const std::vector<uint32_t>& w, const Conv2dShape& s,
                                        const BigNumber& nsq) {
  std::vector<BigNumber> out(s.n_img * s.c_out * s.outHeight() * s.outWidth(), BigNumber(1u));
  for_live_taps(s, [&](size_t o, size_t e, size_t k) { out[o] = (out[o] * pow_mod(x[e], w[k], nsq)) % nsq; });
  return out;
}

static std::vector<BigNumber> plain_conv(const std::vector<uint32_t>& m, const std::vector<uint32_t>& w, const Conv2dShape& s,
                                         const BigNumber& n) {
  std::vector<BigNumber> out(s.n_img * s.c_out * s.outHeight() * s.outWidth(), BigNumber(0u));
  for_live_taps(s, [&](size_t o, size_t e, size_t k) { out[o] = out[o] + BigNumber(w[k]) * BigNumber(m[e]); });
  for (auto& v : out) v = v % n;
  return out;
}

TEST(conv2d_against_host_bignumber_resident_input) {
  ipcl::KeyPair& key = shared_key();
  const Conv2dShape s = shape_of(2, 3, 5, 4, 2, 3, 2, 1, 1, 1, 0);           // everything non-square, padding on one axis
  std::vector<uint32_t> m = random_u32(2 * 3 * 5 * 4, 11), w = random_u32(2 * 3 * 3 * 2, 12);
  for (size_t k = 0; k < 3 * 3 * 2; ++k) w[k] = 0;                           // an all-zero filter: the ciphertext 1
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  EXPECT_TRUE(ct.isDeviceResident());
  ipcl::CipherText y = ipcl::ext::conv2d(ipcl::PlainText(w), ct, s);         // the resident batch is used in place
  EXPECT_TRUE(ct.isDeviceResident());
  EXPECT_TRUE(y.isDeviceResident());
  EXPECT_EQ(s.outHeight(), (size_t)5);
  EXPECT_EQ(s.outWidth(), (size_t)3);
  EXPECT_EQ(y.getSize(), (size_t)(2 * 2 * 5 * 3));
  std::vector<BigNumber> x = ct.getTexts(), want = host_conv(x, w, s, *key.pub_key.getNSQ());
  for (size_t k = 0; k < want.size(); ++k) EXPECT_EQ(y.getElement(k), want[k]);
  for (size_t n = 0; n < 2; ++n)
    for (size_t k = 0; k < 15; ++k) EXPECT_EQ(y.getElement(n * 30 + k), BigNumber(1u));
  std::vector<BigNumber> again = ct.getTexts();                              // x is left unchanged
  for (size_t k = 0; k < x.size(); ++k) EXPECT_EQ(again[k], x[k]);
}

TEST(conv2d_and_conv1d_decrypt_to_the_plain_convolution) {
  ipcl::KeyPair& key = shared_key();
  const BigNumber& n = *key.pub_key.getN();
  const Conv2dShape s = shape_of(3, 2, 7, 3, 4, 3, 3, 2, 1, 1, 1);
  std::vector<uint32_t> m = random_u32(3 * 2 * 7 * 3, 21), w = random_u32(4 * 2 * 3 * 3, 22, 0xfffffu);
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  ipcl::PlainText d = key.priv_key.decrypt(ipcl::ext::conv2d(ipcl::PlainText(w), ct, s));
  std::vector<BigNumber> want = plain_conv(m, w, s, n);
  EXPECT_EQ(d.getSize(), want.size());
  for (size_t k = 0; k < want.size(); ++k) EXPECT_EQ(d.getElement(k), want[k]);
  // conv1d: 2 sequences of 2 channels of 9, 3 filters of 4 taps, stride 2, padding 1 -> [2][3][4]
  std::vector<uint32_t> m1 = random_u32(2 * 2 * 9, 23), w1 = random_u32(3 * 2 * 4, 24, 0xfffffu);
  ipcl::CipherText c1 = key.pub_key.encrypt(ipcl::PlainText(m1));
  ipcl::CipherText y1 = ipcl::ext::conv1d(ipcl::PlainText(w1), c1, 2, 2, 9, 3, 4, 2, 1);
  const Conv2dShape s1 = shape_of(2, 2, 1, 9, 3, 1, 4, 1, 2, 0, 1);
  EXPECT_EQ(y1.getSize(), (size_t)(2 * 3 * 4));
  std::vector<BigNumber> h1 = host_conv(c1.getTexts(), w1, s1, *key.pub_key.getNSQ()), p1 = plain_conv(m1, w1, s1, n);
  ipcl::PlainText d1 = key.priv_key.decrypt(y1);
  for (size_t k = 0; k < h1.size(); ++k) {
    EXPECT_EQ(y1.getElement(k), h1[k]);
    EXPECT_EQ(d1.getElement(k), p1[k]);
  }
  // sum pooling, the caller's reshape: 2 images x 3 channels of 4x4 as 6 images, 2x2 all-ones taps, stride 2
  std::vector<uint32_t> mp = random_u32(2 * 3 * 4 * 4, 25), ones(4, 1u);
  const Conv2dShape sp = shape_of(6, 1, 4, 4, 1, 2, 2, 2, 2);
  ipcl::PlainText dp = key.priv_key.decrypt(ipcl::ext::conv2d(ipcl::PlainText(ones), key.pub_key.encrypt(ipcl::PlainText(mp)), sp));
  std::vector<BigNumber> pp = plain_conv(mp, ones, sp, n);
  EXPECT_EQ(dp.getSize(), (size_t)(6 * 2 * 2));
  for (size_t k = 0; k < pp.size(); ++k) EXPECT_EQ(dp.getElement(k), pp[k]);
}

TEST(two_layers_host_constructed_ciphertext) {
  ipcl::KeyPair& key = shared_key();
  const BigNumber& n = *key.pub_key.getN();
  const Conv2dShape a = shape_of(2, 1, 6, 6, 2, 3, 3, 1, 1, 1, 1), b = shape_of(2, 2, 6, 6, 1, 2, 2, 2, 2);
  std::vector<uint32_t> m = random_u32(2 * 6 * 6, 31, 0xfffffu), wa = random_u32(2 * 3 * 3, 32, 0x1fffu), wb = random_u32(2 * 2 * 2, 33, 0x1fffu);
  std::vector<BigNumber> texts = key.pub_key.encrypt(ipcl::PlainText(m)).getTexts();
  ipcl::CipherText host_ct(key.pub_key, texts);                              // built around host BigNumbers
  ipcl::CipherText y = ipcl::ext::conv2d(ipcl::PlainText(wa), host_ct, a);
  ipcl::CipherText z = ipcl::ext::conv2d(ipcl::PlainText(wb), y, b);         // the first layer's result as it is
  std::vector<BigNumber> hy = host_conv(texts, wa, a, *key.pub_key.getNSQ()), hz = host_conv(hy, wb, b, *key.pub_key.getNSQ());
  EXPECT_EQ(z.getSize(), hz.size());
  for (size_t k = 0; k < hz.size(); ++k) EXPECT_EQ(z.getElement(k), hz[k]);
  // the plain layers (every sum far below n)
  std::vector<BigNumber> py = plain_conv(m, wa, a, n);
  std::vector<BigNumber> pz(hz.size(), BigNumber(0u));
  for_live_taps(b, [&](size_t o, size_t e, size_t k) { pz[o] = pz[o] + BigNumber(wb[k]) * py[e]; });
  ipcl::PlainText d = key.priv_key.decrypt(z);
  for (size_t k = 0; k < pz.size(); ++k) EXPECT_EQ(d.getElement(k), pz[k] % n);
  // the result is an ordinary CipherText: it feeds the operators
  ipcl::CipherText twice = z + z;
  EXPECT_EQ(key.priv_key.decrypt(twice).getElement(1), (d.getElement(1) * 2u) % n);
}

TEST(errors_throw) {
  ipcl::KeyPair& key = shared_key();
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(random_u32(12, 51)));      // 1 x 1 x 3 x 4
  const Conv2dShape ok = shape_of(1, 1, 3, 4, 2, 2, 2);
  bool said = false;
  try {
    ipcl::ext::conv2d(ipcl::PlainText(random_u32(7, 52)), ct, ok);           // 7 weights for 2 filters of 2 x 2
  } catch (const std::runtime_error& e) {
    said = std::string(e.what()).find("conv2d error: Size mismatch!") != std::string::npos;
  }
  EXPECT_TRUE(said);
  const ipcl::PlainText w8(random_u32(8, 53));
  EXPECT_THROW(ipcl::ext::conv2d(w8, ct, shape_of(2, 1, 3, 4, 2, 2, 2)));               // 24 elements asked of 12
  EXPECT_THROW(ipcl::ext::conv2d(w8, ct, shape_of(0, 1, 3, 4, 2, 2, 2)));               // no images
  EXPECT_THROW(ipcl::ext::conv2d(w8, ct, shape_of(1, 1, 3, 4, 2, 2, 2, 0, 1)));         // stride 0
  EXPECT_THROW(ipcl::ext::conv2d(w8, ct, shape_of(1, 1, 3, 4, 2, 2, 2, 1, 1, 2, 0)));   // pad_h >= kh
  EXPECT_THROW(ipcl::ext::conv2d(ipcl::PlainText(random_u32(16, 54)), ct, shape_of(1, 1, 3, 4, 2, 4, 2)));   // kh > h
  EXPECT_THROW(ipcl::ext::conv2d(w8, ipcl::CipherText(), ok));                          // empty CipherText
  EXPECT_THROW(ipcl::ext::conv1d(w8, ct, 1, 1, 12, 2, 5));                              // 8 weights for 2 kernels of 5
  std::vector<BigNumber> neg(8, BigNumber(2u));
  neg[3] = BigNumber(1u) - BigNumber(4u);
  EXPECT_THROW(ipcl::ext::conv2d(ipcl::PlainText(neg), ct, ok));                        // negative weights have no encoding
  EXPECT_EQ(ipcl::ext::conv2d(w8, ct, ok).getSize(), (size_t)(2 * 2 * 3));
  EXPECT_EQ(ipcl::ext::conv1d(w8, ct, 1, 1, 12, 2, 4, 4).getSize(), (size_t)(2 * 3));
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
