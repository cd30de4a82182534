// C++ tests of ipcl::ext::segmentScan (include/ipcl/ext/aggregate.hpp), run on a real MI355X by
// tests/test_gpu_segscan_cpp.py: the fused encrypted segmented prefix sum against host BigNumber arithmetic
// (prod_{u <= t} x[r][u] mod n^2, and u >= t in reverse), against the running sum composed from the reference's operator
// (CipherText::operator+, ipcl/ciphertext.cpp:35-72), through decrypt, on the result of segmentSum without leaving the
// device, with device-resident and host-constructed CipherTexts, and the exceptions of the error paths.
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

static std::vector<BigNumber> host_scan(const std::vector<BigNumber>& x, size_t seg_len, bool reverse, const BigNumber& nsq) {
  std::vector<BigNumber> out(x.size());
  for (size_t r = 0; r < x.size() / seg_len; ++r) {
    BigNumber acc(1u);
    for (size_t i = 0; i < seg_len; ++i) {
      const size_t at = r * seg_len + (reverse ? seg_len - 1 - i : i);
      acc = (acc * x[at]) % nsq;
      out[at] = acc;
    }
  }
  return out;
}

TEST(segment_scan_against_host_bignumber_resident_input) {
  ipcl::KeyPair& key = shared_key();
  const size_t rows = 3, seg_len = 19;                                     // beyond the chunk of 8: every launch of the plan
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(random_u32(rows * seg_len, 11)));
  EXPECT_TRUE(ct.isDeviceResident());
  std::vector<ipcl::CipherText> ys;
  for (bool reverse : {false, true}) {
    ys.push_back(ipcl::ext::segmentScan(ct, seg_len, reverse));            // the resident batch is used in place
    EXPECT_TRUE(ct.isDeviceResident());
    EXPECT_TRUE(ys.back().isDeviceResident());
    EXPECT_EQ(ys.back().getSize(), rows * seg_len);
  }
  const std::vector<BigNumber> texts = ct.getTexts();                      // an accessor: ct holds host values from here on
  for (bool reverse : {false, true}) {
    std::vector<BigNumber> want = host_scan(texts, seg_len, reverse, *key.pub_key.getNSQ());
    for (size_t i = 0; i < want.size(); ++i) EXPECT_EQ(ys[reverse].getElement(i), want[i]);
  }
}

TEST(segment_scan_host_constructed_and_default_direction) {
  ipcl::KeyPair& key = shared_key();
  const size_t rows = 5, seg_len = 4;
  std::vector<BigNumber> texts = key.pub_key.encrypt(ipcl::PlainText(random_u32(rows * seg_len, 21))).getTexts();
  ipcl::CipherText host_ct(key.pub_key, texts);                            // built around host BigNumbers
  ipcl::CipherText y = ipcl::ext::segmentScan(host_ct, seg_len);           // forward by default
  std::vector<BigNumber> want = host_scan(texts, seg_len, false, *key.pub_key.getNSQ());
  for (size_t i = 0; i < want.size(); ++i) EXPECT_EQ(y.getElement(i), want[i]);
}

TEST(segment_scan_decrypts_to_the_cumulative_sums) {
  ipcl::KeyPair& key = shared_key();
  const size_t rows = 2, seg_len = 70;
  std::vector<uint32_t> m = random_u32(rows * seg_len, 31);
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
  ipcl::PlainText f = key.priv_key.decrypt(ipcl::ext::segmentScan(ct, seg_len));
  ipcl::PlainText b = key.priv_key.decrypt(ipcl::ext::segmentScan(ct, seg_len, true));
  for (size_t r = 0; r < rows; ++r) {
    BigNumber acc(0u);
    for (size_t t = 0; t < seg_len; ++t) {
      acc = acc + BigNumber(m[r * seg_len + t]);
      EXPECT_EQ(f.getElement(r * seg_len + t), acc % *key.pub_key.getN());
    }
    acc = BigNumber(0u);
    for (size_t t = seg_len; t-- > 0;) {
      acc = acc + BigNumber(m[r * seg_len + t]);
      EXPECT_EQ(b.getElement(r * seg_len + t), acc % *key.pub_key.getN());
    }
  }
}

TEST(segment_scan_equals_the_composed_operator) {
  ipcl::KeyPair& key = shared_key();
  const size_t n = 9;
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(random_u32(n, 41)));
  ipcl::CipherText y = ipcl::ext::segmentScan(ct, n);
  ipcl::CipherText acc = ct.getCipherText(0);                              // the reference's route: CT + CT, element by element
  EXPECT_EQ(y.getElement(0), acc.getElement(0));
  for (size_t t = 1; t < n; ++t) {
    acc = acc + ct.getCipherText(t);
    EXPECT_EQ(y.getElement(t), acc.getElement(0));
  }
}

TEST(histogram_then_scan_without_leaving_the_device) {
  ipcl::KeyPair& key = shared_key();
  const size_t cols = 120, n_segments = 6, groups = 3;
  std::vector<uint32_t> m = random_u32(cols, 51), ids = random_u32(groups * cols, 52, n_segments);
  ipcl::CipherText h = ipcl::ext::segmentSum(key.pub_key.encrypt(ipcl::PlainText(m)), ids, n_segments, groups);
  EXPECT_TRUE(h.isDeviceResident());
  ipcl::CipherText left = ipcl::ext::segmentScan(h, n_segments), right = ipcl::ext::segmentScan(h, n_segments, true);
  EXPECT_TRUE(h.isDeviceResident());
  EXPECT_TRUE(left.isDeviceResident());
  EXPECT_TRUE(right.isDeviceResident());
  ipcl::PlainText dl = key.priv_key.decrypt(left), dr = key.priv_key.decrypt(right);
  for (size_t g = 0; g < groups; ++g)
    for (size_t t = 0; t < n_segments; ++t) {
      BigNumber lo(0u), hi(0u);                                            // bins 0..t and bins t..: both sides of a split at t
      for (size_t j = 0; j < cols; ++j) {
        if (ids[g * cols + j] <= t) lo = lo + BigNumber(m[j]);
        if (ids[g * cols + j] >= t) hi = hi + BigNumber(m[j]);
      }
      EXPECT_EQ(dl.getElement(g * n_segments + t), lo % *key.pub_key.getN());
      EXPECT_EQ(dr.getElement(g * n_segments + t), hi % *key.pub_key.getN());
    }
  // the result is an ordinary CipherText: it feeds the operators
  ipcl::CipherText both = left + right;
  EXPECT_EQ(both.getSize(), groups * n_segments);
}

TEST(error_paths_throw) {
  ipcl::KeyPair& key = shared_key();
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(random_u32(6, 61)));
  EXPECT_THROW(ipcl::ext::segmentScan(ct, 0));                             // no segment length
  EXPECT_THROW(ipcl::ext::segmentScan(ct, 4));                             // 6 % 4 != 0
  EXPECT_THROW(ipcl::ext::segmentScan(ct, 7, true));                       // longer than the vector
  EXPECT_THROW(ipcl::ext::segmentScan(ipcl::CipherText(), 1));             // empty CipherText
  EXPECT_EQ(ipcl::ext::segmentScan(ct, 6).getSize(), (size_t)6);
  EXPECT_EQ(ipcl::ext::segmentScan(ct, 1, true).getSize(), (size_t)6);
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
