// C++ tests of ipcl::ext::negate / ipcl::ext::subtract (include/ipcl/ext/arith.hpp), run on a real MI355X by
// tests/test_gpu_negate_cpp.py: the batched inversion against host BigNumber arithmetic (x^-1 mod n^2, a * b^-1 mod n^2),
// through decrypt, against the exponentiation by n - 1 that the reference's operator offers (CipherText::operator*,
// ipcl/ciphertext.cpp:83-107), on the result of segmentSum without leaving the device, with device-resident and
// host-constructed CipherTexts, and the exceptions of the error paths.
#include <cstdio>
#include <functional>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "ipcl/ext/aggregate.hpp"
#include "ipcl/ext/arith.hpp"
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

static std::vector<uint32_t> random_u32(size_t n, uint32_t seed, uint32_t mod = 0) {
  std::mt19937 rng(seed);
  std::vector<uint32_t> v(n);
  for (auto& x : v) x = mod ? rng() % mod : rng();
  return v;
}

static ipcl::KeyPair& shared_key() {
  static ipcl::KeyPair key = ipcl::generateKeypair(2048, true);
  return key;
}

TEST(negate_against_host_bignumber_resident_input) {
  ipcl::KeyPair& key = shared_key();
  const size_t n = 70;                                                     // beyond 64: three levels
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(random_u32(n, 11)));
  EXPECT_TRUE(ct.isDeviceResident());
  ipcl::CipherText y = ipcl::ext::negate(ct);                              // the resident batch is used in place
  EXPECT_TRUE(ct.isDeviceResident());
  EXPECT_TRUE(y.isDeviceResident());
  EXPECT_EQ(y.getSize(), n);
  ipcl::CipherText back = ipcl::ext::negate(y);                            // the output of a negate as input
  const BigNumber& nsq = *key.pub_key.getNSQ();
  const std::vector<BigNumber> texts = ct.getTexts();                      // an accessor: ct holds host values from here on
  for (size_t i = 0; i < n; ++i) {
    EXPECT_EQ(y.getElement(i), nsq.InverseMul(texts[i]));
    EXPECT_EQ(back.getElement(i), texts[i]);
  }
}

TEST(subtract_against_host_bignumber_host_constructed) {
  ipcl::KeyPair& key = shared_key();
  const size_t n = 21;
  const BigNumber& nsq = *key.pub_key.getNSQ();
  std::vector<BigNumber> ta = key.pub_key.encrypt(ipcl::PlainText(random_u32(n, 21))).getTexts();
  std::vector<BigNumber> tb = key.pub_key.encrypt(ipcl::PlainText(random_u32(n, 22))).getTexts();
  ipcl::CipherText a(key.pub_key, ta), b(key.pub_key, tb);                 // built around host BigNumbers
  ipcl::CipherText d = ipcl::ext::subtract(a, b);
  EXPECT_TRUE(d.isDeviceResident());
  for (size_t i = 0; i < n; ++i) EXPECT_EQ(d.getElement(i), (ta[i] * nsq.InverseMul(tb[i])) % nsq);
  ipcl::CipherText one(key.pub_key, tb[3]);                                // the broadcast b
  ipcl::CipherText e = ipcl::ext::subtract(a, one);
  EXPECT_EQ(e.getSize(), n);
  const BigNumber inv3 = nsq.InverseMul(tb[3]);
  for (size_t i = 0; i < n; ++i) EXPECT_EQ(e.getElement(i), (ta[i] * inv3) % nsq);
}

TEST(negate_and_subtract_decrypt) {
  ipcl::KeyPair& key = shared_key();
  const size_t n = 9;
  const BigNumber& N = *key.pub_key.getN();
  std::vector<uint32_t> ma = random_u32(n, 31), mb = random_u32(n, 32);
  ma[0] = 0;
  ipcl::CipherText a = key.pub_key.encrypt(ipcl::PlainText(ma)), b = key.pub_key.encrypt(ipcl::PlainText(mb));
  ipcl::PlainText dn = key.priv_key.decrypt(ipcl::ext::negate(a));
  ipcl::PlainText ds = key.priv_key.decrypt(ipcl::ext::subtract(a, b));
  ipcl::PlainText dz = key.priv_key.decrypt(ipcl::ext::subtract(a, a));
  for (size_t i = 0; i < n; ++i) {
    EXPECT_EQ(dn.getElement(i), (N - BigNumber(ma[i])) % N);
    EXPECT_EQ(ds.getElement(i), (N + BigNumber(ma[i]) - BigNumber(mb[i])) % N);
    EXPECT_EQ(dz.getElement(i), BigNumber(0u));
  }
  // the same plaintexts as the reference's route to Enc(-m): CT * PT with n - 1 (other ciphertexts: only the decryption agrees)
  ipcl::PlainText via_mul = key.priv_key.decrypt(a * ipcl::PlainText(N - BigNumber(1u)));
  for (size_t i = 0; i < n; ++i) EXPECT_EQ(via_mul.getElement(i), dn.getElement(i));
}

TEST(sibling_histogram_without_leaving_the_device) {
  ipcl::KeyPair& key = shared_key();
  const size_t cols = 120, n_segments = 6;
  const BigNumber& N = *key.pub_key.getN();
  std::vector<uint32_t> m = random_u32(cols, 51), ids = random_u32(cols, 52, n_segments), in_child = random_u32(cols, 53, 2);
  std::vector<uint32_t> ids_child(cols);
  for (size_t j = 0; j < cols; ++j) ids_child[j] = in_child[j] ? ids[j] : ipcl::ext::kSegmentNone;
  ipcl::CipherText x = key.pub_key.encrypt(ipcl::PlainText(m));
  ipcl::CipherText parent = ipcl::ext::segmentSum(x, ids, n_segments), child = ipcl::ext::segmentSum(x, ids_child, n_segments);
  ipcl::CipherText sibling = ipcl::ext::subtract(parent, child);           // instead of a second histogram
  EXPECT_TRUE(parent.isDeviceResident());
  EXPECT_TRUE(child.isDeviceResident());
  EXPECT_TRUE(sibling.isDeviceResident());
  ipcl::PlainText d = key.priv_key.decrypt(sibling);
  for (size_t s = 0; s < n_segments; ++s) {
    BigNumber want(0u);
    for (size_t j = 0; j < cols; ++j)
      if (ids[j] == s && !in_child[j]) want = want + BigNumber(m[j]);
    EXPECT_EQ(d.getElement(s), want % N);
  }
  ipcl::CipherText again = sibling + child;                                // an ordinary CipherText: it feeds the operators
  ipcl::PlainText dp = key.priv_key.decrypt(again), pp = key.priv_key.decrypt(parent);
  for (size_t s = 0; s < n_segments; ++s) EXPECT_EQ(dp.getElement(s), pp.getElement(s));
}

TEST(error_paths_throw) {
  ipcl::KeyPair& key = shared_key();
  ipcl::CipherText a = key.pub_key.encrypt(ipcl::PlainText(random_u32(6, 61)));
  ipcl::CipherText b4 = key.pub_key.encrypt(ipcl::PlainText(random_u32(4, 62)));
  EXPECT_THROW(ipcl::ext::negate(ipcl::CipherText()));                     // empty CipherText
  EXPECT_THROW(ipcl::ext::subtract(a, b4));                                // 4 is neither 6 nor 1
  EXPECT_THROW(ipcl::ext::subtract(b4, a));
  ipcl::KeyPair other = ipcl::generateKeypair(2048, true);
  ipcl::CipherText c = other.pub_key.encrypt(ipcl::PlainText(random_u32(6, 63)));
  EXPECT_THROW(ipcl::ext::subtract(a, c));                                 // two different public keys
  // not a unit modulo n: no ciphertext, no inverse -- and the next call works
  std::vector<BigNumber> texts = a.getTexts();
  texts[2] = *key.pub_key.getN();
  ipcl::CipherText bad(key.pub_key, texts);
  EXPECT_THROW(ipcl::ext::negate(bad));
  EXPECT_THROW(ipcl::ext::subtract(a, bad));
  EXPECT_EQ(ipcl::ext::negate(a).getSize(), (size_t)6);
  EXPECT_EQ(ipcl::ext::subtract(bad, a).getSize(), (size_t)6);             // (a non-unit may be subtracted FROM)
  EXPECT_EQ(ipcl::ext::subtract(a, b4.getCipherText(0)).getSize(), (size_t)6);
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
