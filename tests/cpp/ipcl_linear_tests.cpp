// C++ tests of ipcl::ext::matVec / dot (include/ipcl/ext/linear.hpp), run on a real MI355X by
// tests/test_gpu_linear_cpp.py: the fused encrypted matrix-vector product against host BigNumber arithmetic
// (prod_j x[j]^w[i][j] mod n^2, square and multiply), against the map composed from the reference's operators
// (CipherText::operator* / operator+, ipcl/ciphertext.cpp:83-106, 35-72), through decrypt, with device-resident and
// host-constructed CipherTexts, and the exception on a size mismatch.
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

TEST(matvec_against_host_bignumber_resident_input) {
  ipcl::KeyPair& key = shared_key();
  const size_t rows = 5, cols = 13;
  std::vector<uint32_t> m = random_u32(cols, 11), w = random_u32(rows * cols, 12);
  w[0] = 0;
  for (size_t j = 0; j < cols; ++j) w[2 * cols + j] = 0;   // an all-zero row: an encryption-free 1
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  EXPECT_TRUE(ct.isDeviceResident());
  ipcl::CipherText y = ipcl::ext::matVec(ipcl::PlainText(w), rows, ct);   // the resident batch is used in place
  EXPECT_TRUE(ct.isDeviceResident());
  EXPECT_TRUE(y.isDeviceResident());
  EXPECT_EQ(y.getSize(), rows);
  const BigNumber nsq = *key.pub_key.getNSQ();
  std::vector<BigNumber> want = host_matvec(ct.getTexts(), w, rows, nsq);
  for (size_t i = 0; i < rows; ++i) EXPECT_EQ(y.getElement(i), want[i]);
  EXPECT_EQ(y.getElement(2), BigNumber(1u));
}

TEST(matvec_host_constructed_ciphertext) {
  ipcl::KeyPair& key = shared_key();
  const size_t rows = 3, cols = 6;
  std::vector<uint32_t> m = random_u32(cols, 21), w = random_u32(rows * cols, 22, 0xffffu);
  std::vector<BigNumber> texts = key.pub_key.encrypt(ipcl::PlainText(m)).getTexts();
  ipcl::CipherText host_ct(key.pub_key, texts);             // built around host BigNumbers
  ipcl::CipherText y = ipcl::ext::matVec(ipcl::PlainText(w), rows, host_ct);
  std::vector<BigNumber> want = host_matvec(texts, w, rows, *key.pub_key.getNSQ());
  for (size_t i = 0; i < rows; ++i) EXPECT_EQ(y.getElement(i), want[i]);
}

TEST(matvec_decrypts_to_the_linear_map) {
  ipcl::KeyPair& key = shared_key();
  const size_t rows = 7, cols = 40;
  std::vector<uint32_t> m = random_u32(cols, 31), w = random_u32(rows * cols, 32);
  ipcl::CipherText y = ipcl::ext::matVec(ipcl::PlainText(w), rows, key.pub_key.encrypt(ipcl::PlainText(m)));
  ipcl::PlainText d = key.priv_key.decrypt(y);
  for (size_t i = 0; i < rows; ++i) {
    BigNumber acc(0u);
    for (size_t j = 0; j < cols; ++j) acc = acc + BigNumber(w[i * cols + j]) * BigNumber(m[j]);
    EXPECT_EQ(d.getElement(i), acc % *key.pub_key.getN());
  }
}

TEST(dot_equals_the_composed_operators) {
  ipcl::KeyPair& key = shared_key();
  const size_t cols = 9;
  std::vector<uint32_t> m = random_u32(cols, 41), w = random_u32(cols, 42);
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  ipcl::CipherText y = ipcl::ext::dot(ipcl::PlainText(w), ct);
  EXPECT_EQ(y.getSize(), (size_t)1);
  ipcl::CipherText terms = ct * ipcl::PlainText(w);          // the reference's route: CT * PT, then CT + CT
  ipcl::CipherText acc = terms.getCipherText(0);
  for (size_t j = 1; j < cols; ++j) acc = acc + terms.getCipherText(j);
  EXPECT_EQ(y.getElement(0), acc.getElement(0));
  // the result is an ordinary CipherText: it feeds the operators and a second layer
  ipcl::CipherText twice = y + y;
  EXPECT_EQ(key.priv_key.decrypt(twice).getElement(0), (key.priv_key.decrypt(y).getElement(0) * 2u) % *key.pub_key.getN());
  ipcl::CipherText z = ipcl::ext::dot(ipcl::PlainText(std::vector<uint32_t>{3u}), y);
  EXPECT_EQ(key.priv_key.decrypt(z).getElement(0), (key.priv_key.decrypt(y).getElement(0) * 3u) % *key.pub_key.getN());
}

TEST(size_mismatch_throws) {
  ipcl::KeyPair& key = shared_key();
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(random_u32(4, 51)));
  EXPECT_THROW(ipcl::ext::matVec(ipcl::PlainText(random_u32(7, 52)), 2, ct));    // 7 != 2 * 4
  EXPECT_THROW(ipcl::ext::matVec(ipcl::PlainText(random_u32(8, 53)), 0, ct));    // no rows
  EXPECT_THROW(ipcl::ext::matVec(ipcl::PlainText(random_u32(8, 54)), 3, ct));    // 8 is not 3 rows
  EXPECT_THROW(ipcl::ext::dot(ipcl::PlainText(random_u32(5, 55)), ct));
  EXPECT_THROW(ipcl::ext::dot(ipcl::PlainText(random_u32(4, 56)), ipcl::CipherText()));   // empty CipherText
  EXPECT_EQ(ipcl::ext::matVec(ipcl::PlainText(random_u32(8, 57)), 2, ct).getSize(), (size_t)2);
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
