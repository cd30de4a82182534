// C++ tests of ipcl::ext::weightedSum / sum (include/ipcl/ext/linear.hpp), run on a real MI355X by
// tests/test_gpu_wsum_cpp.py: the fused encrypted weighted sum across K CipherTexts against host BigNumber arithmetic
// (prod_k x_k[i]^w[k] mod n^2, square and multiply), through decrypt, with device-resident and host-constructed
// CipherTexts in one call, and the exceptions on empty operands, size mismatches and negative weights.  The reference
// composes such a sum from CipherText::operator* / operator+ (ipcl/ciphertext.cpp:83-106, 35-72).
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

static BigNumber pow_mod(const BigNumber& x, const BigNumber& e, const BigNumber& mod) {
  BigNumber acc(1u), base = x % mod;
  std::vector<Ipp32u> words;
  e.num2vec(words);
  for (size_t j = 0; j < words.size(); ++j)
    for (int b = 0; b < 32; ++b) {
      if ((words[j] >> b) & 1u) acc = (acc * base) % mod;
      base = (base * base) % mod;
    }
  return acc;
}

static std::vector<BigNumber> host_wsum(const std::vector<std::vector<BigNumber>>& xs, const std::vector<BigNumber>& w,
                                        const BigNumber& nsq) {
  std::vector<BigNumber> out;
  for (size_t i = 0; i < xs[0].size(); ++i) {
    BigNumber acc(1u);
    for (size_t k = 0; k < xs.size(); ++k) acc = (acc * pow_mod(xs[k][i], w[k], nsq)) % nsq;
    out.push_back(acc);
  }
  return out;
}

TEST(weighted_sum_against_host_bignumber_resident_inputs) {
  ipcl::KeyPair& key = shared_key();
  const size_t count = 21, K = 5;
  std::vector<ipcl::CipherText> xs;
  std::vector<std::vector<uint32_t>> ms;
  for (size_t k = 0; k < K; ++k) {
    ms.push_back(random_u32(count, 10 + (uint32_t)k));
    xs.push_back(key.pub_key.encrypt(ipcl::PlainText(ms.back())));
    EXPECT_TRUE(xs.back().isDeviceResident());
  }
  std::vector<uint32_t> w32 = random_u32(K, 20);
  w32[1] = 0;                                                                // a zero weight contributes nothing
  w32[2] = 1;
  ipcl::CipherText y = ipcl::ext::weightedSum(xs, ipcl::PlainText(w32));     // the resident batches are used in place
  EXPECT_TRUE(y.isDeviceResident());
  for (const auto& x : xs) EXPECT_TRUE(x.isDeviceResident());
  EXPECT_EQ(y.getSize(), count);
  std::vector<std::vector<BigNumber>> texts;
  std::vector<BigNumber> w;
  for (const auto& x : xs) texts.push_back(x.getTexts());
  for (uint32_t v : w32) w.push_back(BigNumber(v));
  std::vector<BigNumber> want = host_wsum(texts, w, *key.pub_key.getNSQ());
  for (size_t i = 0; i < count; ++i) EXPECT_EQ(y.getElement(i), want[i]);
  // through decrypt: sum_k w[k] * m_k[i] mod n
  ipcl::PlainText d = key.priv_key.decrypt(y);
  for (size_t i = 0; i < count; ++i) {
    BigNumber acc(0u);
    for (size_t k = 0; k < K; ++k) acc = acc + BigNumber(w32[k]) * BigNumber(ms[k][i]);
    EXPECT_EQ(d.getElement(i), acc % *key.pub_key.getN());
  }
}

TEST(sum_and_wide_weights_with_host_constructed_ciphertexts) {
  ipcl::KeyPair& key = shared_key();
  const size_t count = 7, K = 4;
  const BigNumber& n = *key.pub_key.getN();
  std::vector<ipcl::CipherText> xs;
  std::vector<std::vector<uint32_t>> ms;
  std::vector<std::vector<BigNumber>> texts;
  for (size_t k = 0; k < K; ++k) {
    ms.push_back(random_u32(count, 30 + (uint32_t)k));
    ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(ms.back()));
    texts.push_back(ct.getTexts());
    if (k % 2) xs.push_back(ipcl::CipherText(key.pub_key, texts.back()));    // built around host BigNumbers
    else xs.push_back(ct);                                                   // device-resident: both kinds in one call
  }
  xs.push_back(xs[0]);                                                       // the same CipherText twice: once per appearance
  texts.push_back(texts[0]);
  ms.push_back(ms[0]);
  ipcl::CipherText s = ipcl::ext::sum(xs);
  EXPECT_EQ(s.getSize(), count);
  ipcl::PlainText ds = key.priv_key.decrypt(s);
  for (size_t i = 0; i < count; ++i) {
    BigNumber acc(0u);
    for (size_t k = 0; k < xs.size(); ++k) acc = acc + BigNumber(ms[k][i]);
    EXPECT_EQ(ds.getElement(i), acc % n);
  }
  // -1 mod n, a 65-bit weight, 1, 0, 3
  const BigNumber two32 = BigNumber(0x80000000u) * BigNumber(2u);
  std::vector<BigNumber> w = {n - BigNumber(1u), two32 * two32 + BigNumber(5u), BigNumber(1u), BigNumber(0u), BigNumber(3u)};
  ipcl::CipherText y = ipcl::ext::weightedSum(xs, ipcl::PlainText(w));
  std::vector<BigNumber> want = host_wsum(texts, w, *key.pub_key.getNSQ());
  for (size_t i = 0; i < count; ++i) EXPECT_EQ(y.getElement(i), want[i]);
  // the result is an ordinary CipherText: it feeds the operators
  ipcl::CipherText twice = y + y;
  EXPECT_EQ(key.priv_key.decrypt(twice).getElement(1), (key.priv_key.decrypt(y).getElement(1) * 2u) % n);
  // all weights zero: encryptions of 0, the ciphertext 1
  ipcl::CipherText z = ipcl::ext::weightedSum(xs, ipcl::PlainText(std::vector<uint32_t>(xs.size(), 0u)));
  for (size_t i = 0; i < count; ++i) EXPECT_EQ(z.getElement(i), BigNumber(1u));
  // one CipherText, weight 1: a copy
  ipcl::CipherText c = ipcl::ext::weightedSum({xs[1]}, ipcl::PlainText(std::vector<uint32_t>{1u}));
  for (size_t i = 0; i < count; ++i) EXPECT_EQ(c.getElement(i), texts[1][i]);
}

TEST(errors_throw) {
  ipcl::KeyPair& key = shared_key();
  ipcl::CipherText a = key.pub_key.encrypt(ipcl::PlainText(random_u32(4, 51)));
  ipcl::CipherText b = key.pub_key.encrypt(ipcl::PlainText(random_u32(4, 52)));
  ipcl::CipherText shorter = key.pub_key.encrypt(ipcl::PlainText(random_u32(3, 53)));
  EXPECT_THROW(ipcl::ext::weightedSum({}, ipcl::PlainText(random_u32(1, 54))));                 // empty xs
  EXPECT_THROW(ipcl::ext::sum({}));
  EXPECT_THROW(ipcl::ext::sum({ipcl::CipherText(), ipcl::CipherText()}));                       // empty CipherTexts
  EXPECT_THROW(ipcl::ext::weightedSum({a, shorter}, ipcl::PlainText(random_u32(2, 55))));       // sizes differ
  EXPECT_THROW(ipcl::ext::sum({a, shorter}));
  EXPECT_THROW(ipcl::ext::weightedSum({a, b}, ipcl::PlainText(random_u32(3, 56))));             // 3 weights for 2 CipherTexts
  EXPECT_THROW(ipcl::ext::weightedSum({a, b}, ipcl::PlainText()));
  std::vector<BigNumber> neg = {BigNumber(5u), BigNumber(1u) - BigNumber(4u)};
  EXPECT_THROW(ipcl::ext::weightedSum({a, b}, ipcl::PlainText(neg)));                           // negative weights have no encoding
  EXPECT_EQ(ipcl::ext::weightedSum({a, b}, ipcl::PlainText(random_u32(2, 57))).getSize(), (size_t)4);
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
