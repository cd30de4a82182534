// C++ tests of ipcl::ext::matMul (include/ipcl/ext/linear.hpp), run on a real MI355X by tests/test_gpu_matmul_cpp.py: the
// fused encrypted matrix product against host BigNumber arithmetic (prod_j x(v, j)^w[i][j] mod n^2, square and multiply)
// in both layouts, against matVec vector by vector, through decrypt, with a device-resident CipherText used in place and a
// host-constructed one, and the exceptions on a size mismatch, empty operands and negative weights.  The reference
// composes such a map from CipherText::operator* / operator+ (ipcl/ciphertext.cpp:83-106, 35-72).
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

// out[v * rows + i] (transposed: out[i * n_vec + v]) = prod_j x(v, j)^w[i * cols + j]
static std::vector<BigNumber> host_matmul(const std::vector<BigNumber>& x, const std::vector<uint32_t>& w, size_t n_vec,
                                          size_t rows, bool transposed, const BigNumber& nsq) {
  const size_t cols = x.size() / n_vec;
  std::vector<BigNumber> out(n_vec * rows);
  for (size_t v = 0; v < n_vec; ++v)
    for (size_t i = 0; i < rows; ++i) {
      BigNumber acc(1u);
      for (size_t j = 0; j < cols; ++j)
        acc = (acc * pow_mod(x[transposed ? j * n_vec + v : v * cols + j], w[i * cols + j], nsq)) % nsq;
      out[transposed ? i * n_vec + v : v * rows + i] = acc;
    }
  return out;
}

TEST(matmul_both_layouts_against_host_bignumber_resident_input) {
  ipcl::KeyPair& key = shared_key();
  const size_t n_vec = 3, cols = 7, rows = 5;
  std::vector<uint32_t> m = random_u32(n_vec * cols, 11), w = random_u32(rows * cols, 12);
  for (size_t j = 0; j < cols; ++j) w[j] = 0;                                // an all-zero row: the ciphertext 1
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  EXPECT_TRUE(ct.isDeviceResident());
  std::vector<ipcl::CipherText> ys;
  for (bool tr : {false, true}) {
    ys.push_back(ipcl::ext::matMul(ipcl::PlainText(w), rows, ct, n_vec, tr));   // the resident batch is used in place
    EXPECT_TRUE(ct.isDeviceResident());
    EXPECT_TRUE(ys.back().isDeviceResident());
    EXPECT_EQ(ys.back().getSize(), n_vec * rows);
  }
  std::vector<BigNumber> x = ct.getTexts();
  for (bool tr : {false, true}) {
    const ipcl::CipherText& y = ys[tr ? 1 : 0];
    std::vector<BigNumber> want = host_matmul(x, w, n_vec, rows, tr, *key.pub_key.getNSQ());
    for (size_t k = 0; k < want.size(); ++k) EXPECT_EQ(y.getElement(k), want[k]);
    for (size_t v = 0; v < n_vec; ++v) EXPECT_EQ(y.getElement(tr ? v : v * rows), BigNumber(1u));
  }
}

TEST(matmul_decrypts_to_the_plain_product) {
  ipcl::KeyPair& key = shared_key();
  const size_t n_vec = 4, cols = 6, rows = 3;
  std::vector<uint32_t> m = random_u32(n_vec * cols, 21), w = random_u32(rows * cols, 22, 0xfffffu);
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  ipcl::PlainText d = key.priv_key.decrypt(ipcl::ext::matMul(ipcl::PlainText(w), rows, ct, n_vec));
  ipcl::PlainText dt = key.priv_key.decrypt(ipcl::ext::matMul(ipcl::PlainText(w), rows, ct, n_vec, true));
  for (size_t v = 0; v < n_vec; ++v)
    for (size_t i = 0; i < rows; ++i) {
      BigNumber acc(0u), acct(0u);
      for (size_t j = 0; j < cols; ++j) {
        acc = acc + BigNumber(w[i * cols + j]) * BigNumber(m[v * cols + j]);
        acct = acct + BigNumber(w[i * cols + j]) * BigNumber(m[j * n_vec + v]);     // the same storage read as [cols][n_vec]
      }
      EXPECT_EQ(d.getElement(v * rows + i), acc % *key.pub_key.getN());
      EXPECT_EQ(dt.getElement(i * n_vec + v), acct % *key.pub_key.getN());
    }
}

TEST(matmul_equals_matvec_per_vector_host_constructed_ciphertext) {
  ipcl::KeyPair& key = shared_key();
  const size_t n_vec = 3, cols = 9, rows = 4;
  std::vector<uint32_t> m = random_u32(n_vec * cols, 31), w = random_u32(rows * cols, 32, 0xffffu);
  std::vector<BigNumber> texts = key.pub_key.encrypt(ipcl::PlainText(m)).getTexts();
  ipcl::CipherText host_ct(key.pub_key, texts);                              // built around host BigNumbers
  ipcl::CipherText y = ipcl::ext::matMul(ipcl::PlainText(w), rows, host_ct, n_vec);
  for (size_t v = 0; v < n_vec; ++v) {
    std::vector<BigNumber> one(texts.begin() + v * cols, texts.begin() + (v + 1) * cols);
    ipcl::CipherText yv = ipcl::ext::matVec(ipcl::PlainText(w), rows, ipcl::CipherText(key.pub_key, one));
    for (size_t i = 0; i < rows; ++i) EXPECT_EQ(y.getElement(v * rows + i), yv.getElement(i));
  }
  // n_vec = 1 is matVec in both layouts; the result is an ordinary CipherText: it feeds the operators
  std::vector<BigNumber> one(texts.begin(), texts.begin() + cols);
  ipcl::CipherText x1(key.pub_key, one);
  ipcl::CipherText a = ipcl::ext::matMul(ipcl::PlainText(w), rows, x1, 1), b = ipcl::ext::matMul(ipcl::PlainText(w), rows, x1, 1, true);
  for (size_t i = 0; i < rows; ++i) EXPECT_EQ(a.getElement(i), b.getElement(i));
  ipcl::CipherText twice = y + y;
  const BigNumber& n = *key.pub_key.getN();
  EXPECT_EQ(key.priv_key.decrypt(twice).getElement(1), (key.priv_key.decrypt(y).getElement(1) * 2u) % n);
}

TEST(errors_throw) {
  ipcl::KeyPair& key = shared_key();
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(random_u32(6, 51)));
  bool said = false;
  try {
    ipcl::ext::matMul(ipcl::PlainText(random_u32(5, 52)), 2, ct, 2);         // 5 weights for 2 rows of 3 columns
  } catch (const std::runtime_error& e) {
    said = std::string(e.what()).find("matMul error: Size mismatch!") != std::string::npos;
  }
  EXPECT_TRUE(said);
  EXPECT_THROW(ipcl::ext::matMul(ipcl::PlainText(random_u32(6, 53)), 2, ct, 4));               // 4 does not divide 6
  EXPECT_THROW(ipcl::ext::matMul(ipcl::PlainText(random_u32(6, 54)), 2, ct, 0));               // no vectors
  EXPECT_THROW(ipcl::ext::matMul(ipcl::PlainText(random_u32(6, 55)), 0, ct, 2));               // no rows
  EXPECT_THROW(ipcl::ext::matMul(ipcl::PlainText(random_u32(6, 56)), 3, ct, 2));               // 3 rows of 3 need 9 weights
  EXPECT_THROW(ipcl::ext::matMul(ipcl::PlainText(random_u32(6, 57)), 2, ipcl::CipherText(), 2));   // empty CipherText
  std::vector<BigNumber> neg = {BigNumber(5u), BigNumber(1u) - BigNumber(4u), BigNumber(2u)};
  EXPECT_THROW(ipcl::ext::matMul(ipcl::PlainText(neg), 1, ct, 2));                             // negative weights have no encoding
  EXPECT_EQ(ipcl::ext::matMul(ipcl::PlainText(random_u32(6, 58)), 2, ct, 2).getSize(), (size_t)4);
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
