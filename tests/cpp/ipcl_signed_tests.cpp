// C++ tests of ipcl::ext::matVecSigned / dotSigned / matMulSigned (include/ipcl/ext/linear.hpp) on the GPU: the signed-weight
// encrypted linear maps against decrypt -- Dec(out) = W * m mod n in host BigNumber arithmetic --, against the route
// composed from two unsigned calls and a subtraction (ipcl::ext::subtract), in both layouts of the matrix product, and their
// errors.  The reference has no signed weights: its route is CipherText::operator*(PlainText) with w mod n
// (ipcl/ciphertext.cpp:83-107), a key-width exponent per term.
#include <cstdint>
#include <cstdio>
#include <functional>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "ipcl/ext/arith.hpp"
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

static ipcl::KeyPair& shared_key() {
  static ipcl::KeyPair key = ipcl::generateKeypair(2048, true);
  return key;
}

// (sum_j w[j] * m[j]) mod n for one row of signed weights
static BigNumber host_dot(const int64_t* w, const std::vector<uint32_t>& m, size_t m0, size_t m_stride, size_t cols, const BigNumber& n) {
  BigNumber pos(0u), neg(0u);
  for (size_t j = 0; j < cols; ++j) {
    const int64_t e = w[j];
    const BigNumber term = BigNumber((uint32_t)(e < 0 ? -e : e)) * BigNumber(m[m0 + j * m_stride]);
    if (e < 0) neg = neg + term;
    else pos = pos + term;
  }
  return (pos % n + n - neg % n) % n;
}

TEST(matvec_signed_against_decrypt) {
  ipcl::KeyPair& key = shared_key();
  const size_t rows = 6, cols = 13;
  std::vector<uint32_t> m = random_u32(cols, 11);
  std::vector<int64_t> w = random_signed(rows * cols, 12);
  for (size_t j = 0; j < cols; ++j) w[2 * cols + j] = 0;    // an all-zero row: the ciphertext 1
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  ipcl::CipherText y = ipcl::ext::matVecSigned(w, rows, ct);
  EXPECT_TRUE(y.isDeviceResident());
  EXPECT_EQ(y.getSize(), rows);
  EXPECT_EQ(y.getElement(2), BigNumber(1u));
  const BigNumber n = *key.pub_key.getN();
  ipcl::PlainText d = key.priv_key.decrypt(y);
  for (size_t i = 0; i < rows; ++i) EXPECT_EQ(d.getElement(i), host_dot(w.data() + i * cols, m, 0, 1, cols, n));
}

TEST(matvec_signed_equals_two_unsigned_calls_and_a_subtraction) {
  ipcl::KeyPair& key = shared_key();
  const size_t rows = 4, cols = 9;
  std::vector<int64_t> w = random_signed(rows * cols, 21);
  std::vector<uint32_t> wp(w.size()), wn(w.size());
  for (size_t k = 0; k < w.size(); ++k) {
    wp[k] = w[k] > 0 ? (uint32_t)w[k] : 0u;
    wn[k] = w[k] < 0 ? (uint32_t)(-w[k]) : 0u;
  }
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(random_u32(cols, 22)));
  ipcl::CipherText y = ipcl::ext::matVecSigned(w, rows, ct);
  ipcl::CipherText z = ipcl::ext::subtract(ipcl::ext::matVec(ipcl::PlainText(wp), rows, ct), ipcl::ext::matVec(ipcl::PlainText(wn), rows, ct));
  for (size_t i = 0; i < rows; ++i) EXPECT_EQ(y.getElement(i), z.getElement(i));
  // a host-constructed CipherText goes the same way
  ipcl::CipherText host(key.pub_key, ct.getTexts());
  ipcl::CipherText yh = ipcl::ext::matVecSigned(w, rows, host);
  for (size_t i = 0; i < rows; ++i) EXPECT_EQ(yh.getElement(i), y.getElement(i));
}

TEST(dot_signed_is_one_row) {
  ipcl::KeyPair& key = shared_key();
  const size_t cols = 7;
  std::vector<uint32_t> m = random_u32(cols, 31);
  std::vector<int64_t> w = random_signed(cols, 32);
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  ipcl::CipherText y = ipcl::ext::dotSigned(w, ct);
  EXPECT_EQ(y.getSize(), (size_t)1);
  EXPECT_EQ(key.priv_key.decrypt(y).getElement(0), host_dot(w.data(), m, 0, 1, cols, *key.pub_key.getN()));
  // wide weights: the whole int64 range
  std::vector<int64_t> wide = {INT64_MIN, INT64_MAX, -1, 0, 1, -((int64_t)1 << 40), (int64_t)1 << 40};
  ipcl::CipherText yw = ipcl::ext::dotSigned(wide, ct);
  // INT64_MIN + INT64_MAX = -1 and the 2^40 terms cancel where m agrees: check through two halves instead
  std::vector<int64_t> a = {INT64_MIN, 0, -1, 0, 1, 0, 0}, b = {0, INT64_MAX, 0, 0, 0, -((int64_t)1 << 40), (int64_t)1 << 40};
  ipcl::CipherText sum = ipcl::ext::dotSigned(a, ct) + ipcl::ext::dotSigned(b, ct);
  EXPECT_EQ(key.priv_key.decrypt(yw).getElement(0), key.priv_key.decrypt(sum).getElement(0));
}

TEST(matmul_signed_both_layouts_against_decrypt) {
  ipcl::KeyPair& key = shared_key();
  const size_t n_vec = 3, rows = 4, cols = 5;
  std::vector<uint32_t> m = random_u32(n_vec * cols, 41);
  std::vector<int64_t> w = random_signed(rows * cols, 42);
  const BigNumber n = *key.pub_key.getN();
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  // default: m read as [n_vec][cols], the result as [n_vec][rows]
  ipcl::PlainText d = key.priv_key.decrypt(ipcl::ext::matMulSigned(w, rows, ct, n_vec));
  EXPECT_EQ(d.getSize(), n_vec * rows);
  for (size_t v = 0; v < n_vec; ++v)
    for (size_t i = 0; i < rows; ++i) EXPECT_EQ(d.getElement(v * rows + i), host_dot(w.data() + i * cols, m, v * cols, 1, cols, n));
  // transposed: m read as [cols][n_vec], the result as [rows][n_vec]
  ipcl::PlainText t = key.priv_key.decrypt(ipcl::ext::matMulSigned(w, rows, ct, n_vec, true));
  for (size_t i = 0; i < rows; ++i)
    for (size_t v = 0; v < n_vec; ++v) EXPECT_EQ(t.getElement(i * n_vec + v), host_dot(w.data() + i * cols, m, v, n_vec, cols, n));
  // one vector is the matvec
  ipcl::CipherText one = key.pub_key.encrypt(ipcl::PlainText(random_u32(cols, 43)));
  ipcl::CipherText y1 = ipcl::ext::matMulSigned(w, rows, one, 1), y2 = ipcl::ext::matVecSigned(w, rows, one);
  for (size_t i = 0; i < rows; ++i) EXPECT_EQ(y1.getElement(i), y2.getElement(i));
}

TEST(signed_errors) {
  ipcl::KeyPair& key = shared_key();
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(random_u32(4, 51)));
  EXPECT_THROW(ipcl::ext::matVecSigned(random_signed(7, 52), 2, ct));    // 7 != 2 * 4
  EXPECT_THROW(ipcl::ext::matVecSigned(random_signed(8, 53), 0, ct));    // no rows
  EXPECT_THROW(ipcl::ext::matVecSigned(random_signed(8, 54), 3, ct));    // 8 is not 3 rows
  EXPECT_THROW(ipcl::ext::dotSigned(random_signed(5, 55), ct));
  EXPECT_THROW(ipcl::ext::dotSigned(random_signed(4, 56), ipcl::CipherText()));   // empty CipherText
  EXPECT_THROW(ipcl::ext::matMulSigned(random_signed(8, 57), 2, ct, 3));          // 3 does not divide 4
  EXPECT_THROW(ipcl::ext::matMulSigned(random_signed(8, 58), 2, ct, 0));
  EXPECT_THROW(ipcl::ext::matMulSigned(random_signed(8, 59), 2, ct, 2));          // 2 vectors of 2: 4 weights wanted
  EXPECT_EQ(ipcl::ext::matMulSigned(random_signed(4, 60), 2, ct, 2).getSize(), (size_t)4);
  // n is no ciphertext: no inverse modulo n^2 -- an error, and the next call is served
  std::vector<BigNumber> texts = ct.getTexts();
  texts[1] = *key.pub_key.getN();
  EXPECT_THROW(ipcl::ext::dotSigned(random_signed(4, 61), ipcl::CipherText(key.pub_key, texts)));
  EXPECT_EQ(ipcl::ext::matVecSigned(random_signed(8, 62), 2, ct).getSize(), (size_t)2);
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
