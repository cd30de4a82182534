// C++ tests of ipcl::ext::sparseMatVec (include/ipcl/ext/linear.hpp), run on a real MI355X by
// tests/test_gpu_spmv_cpp.py: the fused encrypted sparse matrix-vector product against host BigNumber arithmetic
// (prod_t x[col_idx[t]]^w[t] mod n^2 over the CSR entries of a row, square and multiply), against matVec on the same
// matrix written out densely, through decrypt, with device-resident and host-constructed CipherTexts, and the exceptions
// on a size mismatch, empty operands and negative weights.  The reference composes such a map from
// CipherText::operator* / operator+ (ipcl/ciphertext.cpp:83-106, 35-72).
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

static std::vector<BigNumber> host_spmv(const std::vector<BigNumber>& x, const std::vector<uint64_t>& row_ptr,
                                        const std::vector<uint32_t>& col_idx, const std::vector<uint32_t>& w,
                                        const BigNumber& nsq) {
  std::vector<BigNumber> out;
  for (size_t i = 0; i + 1 < row_ptr.size(); ++i) {
    BigNumber acc(1u);
    for (uint64_t t = row_ptr[i]; t < row_ptr[i + 1]; ++t) acc = (acc * pow_mod(x[col_idx[t]], w[t], nsq)) % nsq;
    out.push_back(acc);
  }
  return out;
}

// a ragged CSR: an empty first row, a row over every column (unsorted), a row naming one column three times, short rows
struct Csr { std::vector<uint64_t> row_ptr; std::vector<uint32_t> col_idx; };
static Csr ragged(size_t cols, uint32_t seed) {
  std::mt19937 rng(seed);
  Csr a;
  a.row_ptr.push_back(0);
  a.row_ptr.push_back(0);                                                    // row 0: empty
  for (size_t j = 0; j < cols; ++j) a.col_idx.push_back((uint32_t)((j * 7 + 3) % cols));   // row 1: every column (cols odd to 7)
  a.row_ptr.push_back(a.col_idx.size());
  for (uint32_t c : {2u, 0u, 2u, 5u, 2u}) a.col_idx.push_back(c);           // row 2: column 2 three times
  a.row_ptr.push_back(a.col_idx.size());
  for (size_t i = 0; i < 6; ++i) {                                           // rows 3..8: 0..5 random entries
    for (size_t k = 0; k < i; ++k) a.col_idx.push_back((uint32_t)(rng() % cols));
    a.row_ptr.push_back(a.col_idx.size());
  }
  return a;
}

TEST(spmv_against_host_bignumber_resident_input) {
  ipcl::KeyPair& key = shared_key();
  const size_t cols = 13;
  Csr a = ragged(cols, 10);
  std::vector<uint32_t> m = random_u32(cols, 11), w = random_u32(a.col_idx.size(), 12);
  w[0] = 0;                                                                  // a zero weight contributes 1
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  EXPECT_TRUE(ct.isDeviceResident());
  ipcl::CipherText y = ipcl::ext::sparseMatVec(a.row_ptr, a.col_idx, ipcl::PlainText(w), ct);   // the resident batch is used in place
  EXPECT_TRUE(ct.isDeviceResident());
  EXPECT_TRUE(y.isDeviceResident());
  EXPECT_EQ(y.getSize(), a.row_ptr.size() - 1);
  std::vector<BigNumber> want = host_spmv(ct.getTexts(), a.row_ptr, a.col_idx, w, *key.pub_key.getNSQ());
  for (size_t i = 0; i < want.size(); ++i) EXPECT_EQ(y.getElement(i), want[i]);
  EXPECT_EQ(y.getElement(0), BigNumber(1u));                                 // the empty row
  EXPECT_EQ(y.getElement(3), BigNumber(1u));
}

TEST(spmv_host_constructed_ciphertext) {
  ipcl::KeyPair& key = shared_key();
  const size_t cols = 9;
  Csr a = ragged(cols, 20);
  std::vector<uint32_t> m = random_u32(cols, 21), w = random_u32(a.col_idx.size(), 22, 0xffffu);
  std::vector<BigNumber> texts = key.pub_key.encrypt(ipcl::PlainText(m)).getTexts();
  ipcl::CipherText host_ct(key.pub_key, texts);                              // built around host BigNumbers
  ipcl::CipherText y = ipcl::ext::sparseMatVec(a.row_ptr, a.col_idx, ipcl::PlainText(w), host_ct);
  std::vector<BigNumber> want = host_spmv(texts, a.row_ptr, a.col_idx, w, *key.pub_key.getNSQ());
  for (size_t i = 0; i < want.size(); ++i) EXPECT_EQ(y.getElement(i), want[i]);
}

TEST(spmv_equals_matvec_on_the_dense_matrix_and_decrypts) {
  ipcl::KeyPair& key = shared_key();
  const size_t cols = 20, rows = 6;
  std::mt19937 rng(30);
  Csr a;
  a.row_ptr.push_back(0);
  std::vector<uint32_t> dense(rows * cols, 0u), w;
  for (size_t i = 0; i < rows; ++i) {                                        // duplicate-free rows of 0, 4, 8, ... 20 entries
    for (size_t j = 0; j < cols; ++j)
      if ((j * 3 + i) % 5 < i) {
        a.col_idx.push_back((uint32_t)j);
        w.push_back((uint32_t)rng());
        dense[i * cols + j] = w.back();
      }
    a.row_ptr.push_back(a.col_idx.size());
  }
  std::vector<uint32_t> m = random_u32(cols, 31);
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  ipcl::CipherText ys = ipcl::ext::sparseMatVec(a.row_ptr, a.col_idx, ipcl::PlainText(w), ct);
  ipcl::CipherText yd = ipcl::ext::matVec(ipcl::PlainText(dense), rows, ct);
  for (size_t i = 0; i < rows; ++i) EXPECT_EQ(ys.getElement(i), yd.getElement(i));
  ipcl::PlainText d = key.priv_key.decrypt(ys);
  for (size_t i = 0; i < rows; ++i) {
    BigNumber acc(0u);
    for (size_t j = 0; j < cols; ++j) acc = acc + BigNumber(dense[i * cols + j]) * BigNumber(m[j]);
    EXPECT_EQ(d.getElement(i), acc % *key.pub_key.getN());
  }
  // the result is an ordinary CipherText: it feeds the operators
  ipcl::CipherText twice = ys + ys;
  EXPECT_EQ(key.priv_key.decrypt(twice).getElement(1), (d.getElement(1) * 2u) % *key.pub_key.getN());
}

TEST(errors_throw) {
  ipcl::KeyPair& key = shared_key();
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(random_u32(4, 51)));
  const std::vector<uint64_t> rp = {0, 2, 3};
  const std::vector<uint32_t> ci = {0, 3, 1};
  EXPECT_THROW(ipcl::ext::sparseMatVec(rp, ci, ipcl::PlainText(random_u32(2, 52)), ct));       // 2 weights for 3 entries
  EXPECT_THROW(ipcl::ext::sparseMatVec(rp, {0, 3}, ipcl::PlainText(random_u32(3, 53)), ct));   // row_ptr.back() != col_idx.size()
  EXPECT_THROW(ipcl::ext::sparseMatVec({0}, {}, ipcl::PlainText(random_u32(3, 54)), ct));      // no rows
  EXPECT_THROW(ipcl::ext::sparseMatVec({}, {}, ipcl::PlainText(random_u32(3, 55)), ct));
  EXPECT_THROW(ipcl::ext::sparseMatVec({0, 0}, {}, ipcl::PlainText(), ct));                    // empty weights
  EXPECT_THROW(ipcl::ext::sparseMatVec(rp, ci, ipcl::PlainText(random_u32(3, 56)), ipcl::CipherText()));   // empty CipherText
  EXPECT_THROW(ipcl::ext::sparseMatVec(rp, {0, 4, 1}, ipcl::PlainText(random_u32(3, 57)), ct));            // a column past x
  EXPECT_THROW(ipcl::ext::sparseMatVec({0, 3, 2, 3}, ci, ipcl::PlainText(random_u32(3, 58)), ct));         // row_ptr decreases
  EXPECT_THROW(ipcl::ext::sparseMatVec({1, 2, 3}, ci, ipcl::PlainText(random_u32(3, 59)), ct));            // row_ptr[0] != 0
  std::vector<BigNumber> neg = {BigNumber(5u), BigNumber(1u) - BigNumber(4u), BigNumber(2u)};
  EXPECT_THROW(ipcl::ext::sparseMatVec(rp, ci, ipcl::PlainText(neg), ct));                     // negative weights have no encoding
  EXPECT_EQ(ipcl::ext::sparseMatVec(rp, ci, ipcl::PlainText(random_u32(3, 60)), ct).getSize(), (size_t)2);
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
