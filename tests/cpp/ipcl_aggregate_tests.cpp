// C++ tests of ipcl::ext::segmentSum (include/ipcl/ext/aggregate.hpp), run on a real MI355X by
// tests/test_gpu_aggregate_cpp.py: the fused encrypted segmented sum against host BigNumber arithmetic
// (prod_{j: ids[g][j] == s} x[j] mod n^2), against the sum composed from the reference's operator
// (CipherText::operator+, ipcl/ciphertext.cpp:35-72), through decrypt, for one and several groups, with device-resident
// and host-constructed CipherTexts, and the exceptions of the error paths.
#include <cstdio>
#include <functional>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "ipcl/ext/aggregate.hpp"
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

using ipcl::ext::kSegmentNone;

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

static std::vector<BigNumber> host_segment_sum(const std::vector<BigNumber>& x, const std::vector<uint32_t>& ids,
                                               size_t n_segments, size_t groups, const BigNumber& nsq) {
  const size_t cols = x.size();
  std::vector<BigNumber> out(groups * n_segments, BigNumber(1u));
  for (size_t g = 0; g < groups; ++g)
    for (size_t j = 0; j < cols; ++j) {
      const uint32_t s = ids[g * cols + j];
      if (s != kSegmentNone) out[g * n_segments + s] = (out[g * n_segments + s] * x[j]) % nsq;
    }
  return out;
}

TEST(segment_sum_against_host_bignumber_resident_input) {
  ipcl::KeyPair& key = shared_key();
  const size_t cols = 29, n_segments = 5;
  std::vector<uint32_t> m = random_u32(cols, 11), ids = random_u32(cols, 12, 4);   // segment 4 stays empty
  ids[3] = kSegmentNone;
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  EXPECT_TRUE(ct.isDeviceResident());
  ipcl::CipherText y = ipcl::ext::segmentSum(ct, ids, n_segments);        // the resident batch is used in place
  EXPECT_TRUE(ct.isDeviceResident());
  EXPECT_TRUE(y.isDeviceResident());
  EXPECT_EQ(y.getSize(), n_segments);
  std::vector<BigNumber> want = host_segment_sum(ct.getTexts(), ids, n_segments, 1, *key.pub_key.getNSQ());
  for (size_t i = 0; i < n_segments; ++i) EXPECT_EQ(y.getElement(i), want[i]);
  EXPECT_EQ(y.getElement(4), BigNumber(1u));
}

TEST(segment_sum_several_groups_host_constructed) {
  ipcl::KeyPair& key = shared_key();
  const size_t cols = 17, n_segments = 3, groups = 4;
  std::vector<uint32_t> m = random_u32(cols, 21), ids = random_u32(groups * cols, 22, 3);
  for (size_t j = 0; j < cols; ++j) ids[2 * cols + j] = kSegmentNone;    // a group that takes no element: all ones
  std::vector<BigNumber> texts = key.pub_key.encrypt(ipcl::PlainText(m)).getTexts();
  ipcl::CipherText host_ct(key.pub_key, texts);                           // built around host BigNumbers
  ipcl::CipherText y = ipcl::ext::segmentSum(host_ct, ids, n_segments, groups);
  EXPECT_EQ(y.getSize(), groups * n_segments);
  std::vector<BigNumber> want = host_segment_sum(texts, ids, n_segments, groups, *key.pub_key.getNSQ());
  for (size_t i = 0; i < want.size(); ++i) EXPECT_EQ(y.getElement(i), want[i]);
  for (size_t s = 0; s < n_segments; ++s) EXPECT_EQ(y.getElement(2 * n_segments + s), BigNumber(1u));
}

TEST(segment_sum_decrypts_to_the_group_sums) {
  ipcl::KeyPair& key = shared_key();
  const size_t cols = 300, n_segments = 7, groups = 2;
  std::vector<uint32_t> m = random_u32(cols, 31), ids = random_u32(groups * cols, 32, n_segments);
  for (size_t j = 0; j < cols; ++j)
    if (j % 10) ids[j] = 0;                                               // the first group: nine tenths in one segment
  ipcl::CipherText y = ipcl::ext::segmentSum(key.pub_key.encrypt(ipcl::PlainText(m)), ids, n_segments, groups);
  ipcl::PlainText d = key.priv_key.decrypt(y);
  for (size_t g = 0; g < groups; ++g)
    for (size_t s = 0; s < n_segments; ++s) {
      BigNumber acc(0u);
      for (size_t j = 0; j < cols; ++j)
        if (ids[g * cols + j] == s) acc = acc + BigNumber(m[j]);
      EXPECT_EQ(d.getElement(g * n_segments + s), acc % *key.pub_key.getN());
    }
}

TEST(segment_sum_equals_the_composed_operator) {
  ipcl::KeyPair& key = shared_key();
  const size_t cols = 11, n_segments = 3;
  std::vector<uint32_t> m = random_u32(cols, 41), ids = random_u32(cols, 42, n_segments);
  ids[0] = 0; ids[1] = 1; ids[2] = 2;                                     // no empty segment
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  ipcl::CipherText y = ipcl::ext::segmentSum(ct, ids, n_segments);
  for (size_t s = 0; s < n_segments; ++s) {                               // the reference's route: CT + CT, element by element
    bool first = true;
    ipcl::CipherText acc;
    for (size_t j = 0; j < cols; ++j) {
      if (ids[j] != s) continue;
      acc = first ? ct.getCipherText(j) : acc + ct.getCipherText(j);
      first = false;
    }
    EXPECT_EQ(y.getElement(s), acc.getElement(0));
  }
  // the result is an ordinary CipherText: it feeds the operators and a second segmented sum
  ipcl::CipherText twice = y + y;
  for (size_t s = 0; s < n_segments; ++s)
    EXPECT_EQ(key.priv_key.decrypt(twice).getElement(s), (key.priv_key.decrypt(y).getElement(s) * 2u) % *key.pub_key.getN());
  ipcl::CipherText total = ipcl::ext::segmentSum(y, std::vector<uint32_t>(n_segments, 0u), 1);
  BigNumber sum(0u);
  for (uint32_t v : m) sum = sum + BigNumber(v);
  EXPECT_EQ(key.priv_key.decrypt(total).getElement(0), sum % *key.pub_key.getN());
}

TEST(error_paths_throw) {
  ipcl::KeyPair& key = shared_key();
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(random_u32(4, 51)));
  EXPECT_THROW(ipcl::ext::segmentSum(ct, {0, 1, 0}, 2));                  // 3 ids for 4 elements
  EXPECT_THROW(ipcl::ext::segmentSum(ct, {0, 1, 0, 1, 0, 1, 0}, 2, 2));   // 7 != 2 * 4
  EXPECT_THROW(ipcl::ext::segmentSum(ct, {0, 1, 0, 1}, 0));               // no segments
  EXPECT_THROW(ipcl::ext::segmentSum(ct, {0, 1, 0, 1}, 2, 0));            // no groups
  EXPECT_THROW(ipcl::ext::segmentSum(ct, {0, 1, 2, 1}, 2));               // id out of range
  EXPECT_THROW(ipcl::ext::segmentSum(ipcl::CipherText(), {}, 2));         // empty CipherText
  EXPECT_EQ(ipcl::ext::segmentSum(ct, {0, 1, kSegmentNone, 1}, 2).getSize(), (size_t)2);
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
