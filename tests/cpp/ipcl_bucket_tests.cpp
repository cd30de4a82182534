// C++ tests of ipcl::ext::matVecBucket (include/ipcl/ext/linear.hpp), run on a real MI355X by
// tests/test_gpu_bucket_cpp.py: the bucket-method encrypted matrix-vector product against host BigNumber arithmetic
// (prod_j x[j]^w[i][j] mod n^2, square and multiply), against matVec on the same operands, through decrypt -- a signed
// weight passed as n - w among them --, with device-resident and host-constructed CipherTexts, and the exceptions on a
// size mismatch, empty operands and negative weights.  The reference composes such a map from CipherText::operator* /
// operator+ (ipcl/ciphertext.cpp:83-106, 35-72).
#include <cstdio>
#include <functional>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

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

static std::vector<BigNumber> host_matvec(const std::vector<BigNumber>& x, const std::vector<uint32_t>& w, size_t rows,
                                          const BigNumber& nsq) {
  const size_t cols = x.size();
  std::vector<BigNumber> out;
  for (size_t i = 0; i < rows; ++i) {
    BigNumber acc(1u);
    for (size_t j = 0; j < cols; ++j) acc = (acc * pow_mod(x[j], w[i * cols + j], nsq)) % nsq;
    out.push_back(acc);
  }
  return out;
}

TEST(bucket_against_host_bignumber_resident_input) {
  ipcl::KeyPair& key = shared_key();
  const size_t cols = 67, rows = 3;
  std::vector<uint32_t> m = random_u32(cols, 11), w = random_u32(rows * cols, 12);
  w[0] = 0;                                                                  // a zero weight contributes 1
  for (size_t j = 0; j < cols; ++j) w[2 * cols + j] = 0;                     // an all-zero row: the ciphertext 1
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  EXPECT_TRUE(ct.isDeviceResident());
  ipcl::CipherText y = ipcl::ext::matVecBucket(ipcl::PlainText(w), rows, ct);   // the resident batch is used in place
  EXPECT_TRUE(ct.isDeviceResident());
  EXPECT_TRUE(y.isDeviceResident());
  EXPECT_EQ(y.getSize(), rows);
  std::vector<BigNumber> want = host_matvec(ct.getTexts(), w, rows, *key.pub_key.getNSQ());
  for (size_t i = 0; i < rows; ++i) EXPECT_EQ(y.getElement(i), want[i]);
  EXPECT_EQ(y.getElement(2), BigNumber(1u));
}

TEST(bucket_host_constructed_ciphertext) {
  ipcl::KeyPair& key = shared_key();
  const size_t cols = 9;
  std::vector<uint32_t> m = random_u32(cols, 21), w = random_u32(cols, 22, 0xffffu);
  std::vector<BigNumber> texts = key.pub_key.encrypt(ipcl::PlainText(m)).getTexts();
  ipcl::CipherText host_ct(key.pub_key, texts);                              // built around host BigNumbers
  ipcl::CipherText y = ipcl::ext::matVecBucket(ipcl::PlainText(w), 1, host_ct);
  std::vector<BigNumber> want = host_matvec(texts, w, 1, *key.pub_key.getNSQ());
  EXPECT_EQ(y.getElement(0), want[0]);
}

TEST(bucket_equals_matvec_and_decrypts) {
  ipcl::KeyPair& key = shared_key();
  const size_t cols = 300, rows = 2;
  std::vector<uint32_t> m = random_u32(cols, 31), w = random_u32(rows * cols, 32);
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  ipcl::CipherText yb = ipcl::ext::matVecBucket(ipcl::PlainText(w), rows, ct);
  ipcl::CipherText yd = ipcl::ext::matVec(ipcl::PlainText(w), rows, ct);
  for (size_t i = 0; i < rows; ++i) EXPECT_EQ(yb.getElement(i), yd.getElement(i));
  ipcl::PlainText d = key.priv_key.decrypt(yb);
  for (size_t i = 0; i < rows; ++i) {
    BigNumber acc(0u);
    for (size_t j = 0; j < cols; ++j) acc = acc + BigNumber(w[i * cols + j]) * BigNumber(m[j]);
    EXPECT_EQ(d.getElement(i), acc % *key.pub_key.getN());
  }
  // the result is an ordinary CipherText: it feeds the operators
  ipcl::CipherText twice = yb + yb;
  EXPECT_EQ(key.priv_key.decrypt(twice).getElement(1), (d.getElement(1) * 2u) % *key.pub_key.getN());
}

TEST(bucket_signed_weights_as_w_mod_n) {
  ipcl::KeyPair& key = shared_key();
  const BigNumber& n = *key.pub_key.getN();
  std::vector<uint32_t> m = random_u32(3, 41);
  std::vector<BigNumber> w = {n - BigNumber(1u), BigNumber(5u), n - BigNumber(7u)};     // -1, 5, -7
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  ipcl::PlainText d = key.priv_key.decrypt(ipcl::ext::matVecBucket(ipcl::PlainText(w), 1, ct));
  BigNumber pos = BigNumber(5u) * BigNumber(m[1]), neg = BigNumber(m[0]) + BigNumber(7u) * BigNumber(m[2]);
  EXPECT_EQ(d.getElement(0), (pos + n * BigNumber(8u) - neg) % n);
}

TEST(errors_throw) {
  ipcl::KeyPair& key = shared_key();
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(random_u32(4, 51)));
  EXPECT_THROW(ipcl::ext::matVecBucket(ipcl::PlainText(random_u32(7, 52)), 2, ct));            // 7 weights for 2 x 4
  EXPECT_THROW(ipcl::ext::matVecBucket(ipcl::PlainText(random_u32(8, 53)), 0, ct));            // no rows
  EXPECT_THROW(ipcl::ext::matVecBucket(ipcl::PlainText(random_u32(8, 54)), 3, ct));            // rows does not divide
  EXPECT_THROW(ipcl::ext::matVecBucket(ipcl::PlainText(), 1, ct));                             // empty weights
  EXPECT_THROW(ipcl::ext::matVecBucket(ipcl::PlainText(random_u32(4, 55)), 1, ipcl::CipherText()));   // empty CipherText
  std::vector<BigNumber> neg = {BigNumber(5u), BigNumber(1u) - BigNumber(4u), BigNumber(2u), BigNumber(3u)};
  EXPECT_THROW(ipcl::ext::matVecBucket(ipcl::PlainText(neg), 1, ct));                          // negative weights have no encoding
  EXPECT_THROW(ipcl::ext::matVec(ipcl::PlainText(neg), 1, ct));                                // (as matVec)
  EXPECT_EQ(ipcl::ext::matVecBucket(ipcl::PlainText(random_u32(8, 56)), 2, ct).getSize(), (size_t)2);
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
