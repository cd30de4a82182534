// C++ tests of ipcl::ext::gather / concat / slice (include/ipcl/ext/index.hpp) and of CipherText::rotate on a
// device-resident text, run on a real MI355X by tests/test_gpu_index_cpp.py: against host vectors after decrypt, rotate on a
// resident product against rotate on a host-built copy (the reference's host rotation, ipcl/ciphertext.cpp:117-133), the
// chain rotate -> operator+ -> decrypt, the reference's messages for the single-element and over-shift errors, and the host
// path for a text whose host copy is current.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "ipcl/ext/index.hpp"
#include "ipcl/ipcl.hpp"
#include "pgpu.h"

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
// the exception's text holds `text`
#define EXPECT_THROW_MSG(stmt, text)                                                              \
  do {                                                                                            \
    std::string what_;                                                                            \
    try { stmt; } catch (const std::runtime_error& e_) { what_ = e_.what(); }                     \
    EXPECT_TRUE(what_.find(text) != std::string::npos);                                           \
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

using ipcl::ext::kGatherOne;

TEST(gather_concat_slice_against_host_vectors_after_decrypt) {
  ipcl::KeyPair& key = shared_key();
  const std::vector<uint32_t> ma = random_u32(23, 11), mb = random_u32(1, 12), mc = random_u32(40, 13);
  ipcl::CipherText a = key.pub_key.encrypt(ipcl::PlainText(ma)), b = key.pub_key.encrypt(ipcl::PlainText(mb)),
                   c = key.pub_key.encrypt(ipcl::PlainText(mc));
  EXPECT_TRUE(a.isDeviceResident());
  std::vector<uint32_t> all(ma);
  all.insert(all.end(), mb.begin(), mb.end());
  all.insert(all.end(), mc.begin(), mc.end());
  all.insert(all.end(), ma.begin(), ma.end());                              // a named twice
  // gather from one text: the reversal, repeats, the sentinel
  std::vector<uint64_t> idx = {22, 0, kGatherOne, 7, 7, 21, kGatherOne};
  ipcl::CipherText g = ipcl::ext::gather(a, idx);
  EXPECT_TRUE(g.isDeviceResident());
  EXPECT_TRUE(a.isDeviceResident());                                        // the resident batch was used in place
  EXPECT_EQ(g.getSize(), idx.size());
  ipcl::PlainText dg = key.priv_key.decrypt(g);
  for (size_t i = 0; i < idx.size(); ++i) EXPECT_EQ(dg.getElement(i), BigNumber(idx[i] == kGatherOne ? 0u : ma[idx[i]]));
  // concat, and gather across several texts
  const std::vector<const ipcl::CipherText*> xs = {&a, &b, &c, &a};
  ipcl::CipherText cat = ipcl::ext::concat(xs);
  EXPECT_TRUE(cat.isDeviceResident());
  EXPECT_EQ(cat.getSize(), all.size());
  ipcl::PlainText dc = key.priv_key.decrypt(cat);
  for (size_t i = 0; i < all.size(); ++i) EXPECT_EQ(dc.getElement(i), BigNumber(all[i]));
  std::vector<uint64_t> across;
  for (size_t i = 0; i < all.size(); ++i) across.push_back(all.size() - 1 - i);
  across.push_back(kGatherOne);
  across.push_back(23);
  ipcl::PlainText dx = key.priv_key.decrypt(ipcl::ext::gather(xs, across));
  for (size_t i = 0; i < across.size(); ++i) EXPECT_EQ(dx.getElement(i), BigNumber(across[i] == kGatherOne ? 0u : all[across[i]]));
  // slices: a contiguous part, strides, one element, the column of [8][5]
  struct { size_t start, count, step; } cuts[] = {{0, 40, 1}, {3, 10, 1}, {39, 1, 1}, {0, 20, 2}, {4, 6, 7}, {2, 8, 5}};
  for (const auto& cut : cuts) {
    ipcl::CipherText s = ipcl::ext::slice(c, cut.start, cut.count, cut.step);
    EXPECT_TRUE(s.isDeviceResident());
    EXPECT_EQ(s.getSize(), cut.count);
    ipcl::PlainText ds = key.priv_key.decrypt(s);
    for (size_t i = 0; i < cut.count; ++i) EXPECT_EQ(ds.getElement(i), BigNumber(mc[cut.start + i * cut.step]));
  }
  EXPECT_EQ(ipcl::ext::slice(c, 5, 3).getSize(), (size_t)3);                // step defaults to 1
  // the results are ordinary CipherTexts: they feed the operators
  ipcl::PlainText sum = key.priv_key.decrypt(g + ipcl::ext::gather(a, idx));
  for (size_t i = 0; i < idx.size(); ++i) EXPECT_EQ(sum.getElement(i), BigNumber(idx[i] == kGatherOne ? 0u : ma[idx[i]]) * BigNumber(2u));
}

TEST(host_only_texts_are_uploaded) {
  ipcl::KeyPair& key = shared_key();
  const std::vector<uint32_t> m = random_u32(9, 21);
  const std::vector<BigNumber> texts = key.pub_key.encrypt(ipcl::PlainText(m)).getTexts();
  ipcl::CipherText h(key.pub_key, texts), h2(key.pub_key, texts);           // built around host BigNumbers
  std::vector<uint64_t> idx = {8, kGatherOne, 0, 4};
  ipcl::CipherText g = ipcl::ext::gather(h, idx);
  EXPECT_TRUE(g.isDeviceResident());
  for (size_t i = 0; i < idx.size(); ++i) EXPECT_EQ(g.getElement(i), idx[i] == kGatherOne ? BigNumber(1u) : texts[idx[i]]);
  ipcl::CipherText cat = ipcl::ext::concat({&h, &h2});
  EXPECT_EQ(cat.getSize(), (size_t)18);
  for (size_t i = 0; i < 18; ++i) EXPECT_EQ(cat.getElement(i), texts[i % 9]);
  ipcl::CipherText s = ipcl::ext::slice(h, 1, 4, 2);
  for (size_t i = 0; i < 4; ++i) EXPECT_EQ(s.getElement(i), texts[1 + 2 * i]);
}

TEST(rotate_on_a_resident_product_equals_rotate_on_a_host_copy) {
  ipcl::KeyPair& key = shared_key();
  const size_t n = 10;
  const std::vector<uint32_t> ma = random_u32(n, 31), mb = random_u32(n, 32);
  ipcl::CipherText prod = key.pub_key.encrypt(ipcl::PlainText(ma)) * ipcl::PlainText(mb);    // a resident product
  EXPECT_TRUE(prod.isDeviceResident());
  ipcl::CipherText copy(prod);                                              // shares the device batch
  const std::vector<BigNumber> texts = copy.getTexts();                     // an accessor: `copy` holds host values from here on
  ipcl::CipherText host(key.pub_key, texts);                                // a host-built copy
  EXPECT_TRUE(!host.isDeviceResident());
  // on a pool of more than one GPU (the runner's second pass) rows are not gathered: rotate takes the host path, as before
  const bool pooled = pgpu_pool_size() > 1;
  if (const char* e = std::getenv("IPCL_EXPECT_POOL")) EXPECT_EQ(pgpu_pool_size(), std::atoi(e));
  for (int shift : {-3, 0, 1, (int)n, -(int)n, 9, -1}) {
    ipcl::CipherText r = prod.rotate(shift);
    EXPECT_EQ(prod.isDeviceResident(), !pooled);
    EXPECT_EQ(r.isDeviceResident(), !pooled);                               // one GPU: rotated on the device, still resident
    ipcl::CipherText want = host.rotate(shift);                             // the host path, as before
    EXPECT_TRUE(!want.isDeviceResident());
    EXPECT_EQ(r.getSize(), n);
    for (size_t i = 0; i < n; ++i) EXPECT_EQ(r.getElement(i), want.getElement(i));
    // a text that still holds its device batch but whose host copy is current: the host path too
    ipcl::CipherText rc = copy.rotate(shift);
    EXPECT_TRUE(!copy.isDeviceResident());
    EXPECT_TRUE(!rc.isDeviceResident());
    for (size_t i = 0; i < n; ++i) EXPECT_EQ(rc.getElement(i), want.getElement(i));
  }
  // positive shift moves elements towards higher indices
  ipcl::CipherText r1 = prod.rotate(1);
  EXPECT_EQ(r1.getElement(1), texts[0]);
  EXPECT_EQ(r1.getElement(0), texts[n - 1]);
  // rotate -> operator+ -> decrypt
  const BigNumber& N = *key.pub_key.getN();
  ipcl::PlainText d = key.priv_key.decrypt(prod.rotate(-3) + prod);
  for (size_t i = 0; i < n; ++i) {
    const size_t j = (i + 3) % n;
    EXPECT_EQ(d.getElement(i), (BigNumber(ma[j]) * BigNumber(mb[j]) + BigNumber(ma[i]) * BigNumber(mb[i])) % N);
  }
}

TEST(rotate_keeps_the_reference_messages) {
  ipcl::KeyPair& key = shared_key();
  ipcl::CipherText one = key.pub_key.encrypt(ipcl::PlainText(random_u32(1, 41)));
  ipcl::CipherText six = key.pub_key.encrypt(ipcl::PlainText(random_u32(6, 42)));
  EXPECT_TRUE(one.isDeviceResident());
  EXPECT_TRUE(six.isDeviceResident());
  EXPECT_THROW_MSG(one.rotate(1), "rotate: Cannot rotate single CipherText");
  EXPECT_THROW_MSG(one.rotate(0), "rotate: Cannot rotate single CipherText");
  EXPECT_THROW_MSG(six.rotate(7), "rotate: Cannot shift more than the test size");
  EXPECT_THROW_MSG(six.rotate(-7), "rotate: Cannot shift more than the test size");
  EXPECT_EQ(six.isDeviceResident(), pgpu_pool_size() == 1);                 // (the host path of a pool downloads first)
  // the same from the host path
  ipcl::CipherText host1(key.pub_key, one.getTexts()), host6(key.pub_key, six.getTexts());
  EXPECT_THROW_MSG(host1.rotate(1), "rotate: Cannot rotate single CipherText");
  EXPECT_THROW_MSG(host6.rotate(7), "rotate: Cannot shift more than the test size");
  EXPECT_EQ(host6.rotate(6).getSize(), (size_t)6);
}

TEST(error_paths_throw) {
  ipcl::KeyPair& key = shared_key();
  ipcl::CipherText a = key.pub_key.encrypt(ipcl::PlainText(random_u32(6, 51)));
  ipcl::CipherText empty;
  EXPECT_THROW(ipcl::ext::gather(a, {}));                                   // empty index list
  EXPECT_THROW(ipcl::ext::gather(a, {6}));                                  // out of range
  EXPECT_THROW(ipcl::ext::gather(a, {0, kGatherOne - 1}));
  EXPECT_THROW(ipcl::ext::gather(empty, {0}));                              // empty CipherText
  EXPECT_THROW(ipcl::ext::gather(std::vector<const ipcl::CipherText*>{}, {0}));
  EXPECT_THROW(ipcl::ext::concat({}));
  EXPECT_THROW(ipcl::ext::concat({&a, nullptr}));
  EXPECT_THROW(ipcl::ext::concat({&a, &empty}));
  EXPECT_THROW(ipcl::ext::slice(a, 0, 3, 0));                               // step == 0
  EXPECT_THROW(ipcl::ext::slice(a, 0, 0, 1));
  EXPECT_THROW(ipcl::ext::slice(a, 6, 1, 1));                               // past the end
  EXPECT_THROW(ipcl::ext::slice(a, 0, 7, 1));
  EXPECT_THROW(ipcl::ext::slice(a, 1, 4, 2));
  ipcl::KeyPair other = ipcl::generateKeypair(2048, true);
  ipcl::CipherText c = other.pub_key.encrypt(ipcl::PlainText(random_u32(6, 52)));
  EXPECT_THROW_MSG(ipcl::ext::concat({&a, &c}), "2 different public keys detected!");
  EXPECT_THROW_MSG(ipcl::ext::gather({&a, &c}, {0, 7}), "2 different public keys detected!");
  // a resident result beside a host-built text: different layouts, no conversion inside the call -- the GPU layer says so
  ipcl::CipherText host(key.pub_key, a.getTexts());
  ipcl::CipherText b = key.pub_key.encrypt(ipcl::PlainText(random_u32(6, 53)));
  EXPECT_THROW(ipcl::ext::concat({&b, &host}));
  EXPECT_EQ(ipcl::ext::concat({&b, &b}).getSize(), (size_t)12);             // and the next call works
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
