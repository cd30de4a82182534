// CPU unit test of the plan of the encrypted segmented prefix sum (pailliercryptolib_amd/csrc/policy.cpp: segscan_*): the
// chunk rule, the level and product counts and the descriptors of every level -- the up-sweep SegsumChunks and the scan
// descriptors are EXECUTED here on small integers modulo a prime, level by level in the order the call launches them,
// and the result is compared with the naive prefix / suffix product.  Pure host logic -- built with g++ from policy.cpp
// alone, no device, no HIP call.  In the reference such a running sum is composed from CipherText::operator+
// (ipcl/ciphertext.cpp:35-72) element by element; the rule is documented in DESIGN.md ("Encrypted segmented prefix sum").
//
// `segscan_policy_tests plan` reads "rows seg_len chunk reverse" from standard input and prints the plan
// (tests/test_segscan_model.py replays it in plain integers).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "policy.hpp"

namespace pol = pgpu::policy;
using pgpu::kSegscanNoCarry;
using pgpu::kSegsumPartial;
using pgpu::SegscanChunk;
using pgpu::SegsumChunk;
static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      ++g_failed;                                                          \
      std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);          \
    }                                                                      \
  } while (0)

static const uint64_t P = 1000003;   // products of values below P stay below 2^40

// Executes a plan the way pgpu_batch_ct_segment_scan launches it and checks what every plan must hold.
static void check_plan(size_t rows, size_t seg_len, int chunk, bool reverse) {
  pol::SegscanPlan plan;
  pol::segscan_plan(rows, seg_len, chunk, reverse, &plan);
  const size_t count = rows * seg_len, nl = plan.levels.size();
  CHECK(plan.chunk == chunk);
  CHECK((int)nl == pol::segscan_levels(chunk, seg_len) && nl >= 1);
  CHECK((nl == 1) == (seg_len <= (size_t)chunk));
  CHECK(pol::segscan_fits(chunk, rows, seg_len));
  std::vector<uint64_t> x(count);
  for (size_t i = 0; i < count; ++i) x[i] = 2 + (i * 7919 + rows * 31 + seg_len) % (P - 2);
  // in[l]: what level l reads (x, or the totals of level l - 1); res[l]: what it writes (the result, or the carries)
  std::vector<std::vector<uint64_t>> in(nl), res(nl);
  std::vector<std::vector<int>> res_written(nl);
  in[0] = x;
  size_t executed = 0;
  for (size_t l = 0; l < nl; ++l) {
    const auto& lv = plan.levels[l];
    CHECK(lv.rows == rows && lv.seg_len * rows == in[l].size());
    CHECK(lv.reverse == (l == 0 && reverse));
    CHECK((l + 1 == nl) == lv.up.empty() && (l + 1 == nl) == (lv.totals == 0));
    if (l + 1 == nl) break;
    // the up-sweep: segsum_kernel with perm == null, every descriptor a row of the totals
    std::vector<uint64_t> totals(lv.totals, 0);
    std::vector<int> written(lv.totals, 0);
    size_t level_products = 0;
    for (const SegsumChunk& c : lv.up) {
      CHECK((c.dst & kSegsumPartial) != 0);
      const size_t r = c.dst & ~kSegsumPartial;
      CHECK(r < lv.totals && c.len >= 1 && c.len <= (uint32_t)chunk);
      CHECK(c.begin + c.len <= in[l].size());
      if (r >= lv.totals || c.begin + c.len > in[l].size() || c.len == 0) continue;
      uint64_t acc = in[l][c.begin];
      for (uint32_t t = 1; t < c.len; ++t, ++level_products) acc = acc * in[l][c.begin + t] % P;
      totals[r] = acc;
      ++written[r];
    }
    for (int w : written) CHECK(w == 1);
    executed += level_products;
    CHECK(lv.totals == rows * plan.levels[l + 1].seg_len);
    in[l + 1] = totals;
  }
  for (size_t l = nl; l-- > 0;) {
    const auto& lv = plan.levels[l];
    const size_t n = in[l].size();
    res[l].assign(n, 0);
    res_written[l].assign(n, 0);
    size_t level_products = 0;
    for (size_t i = 0; i < lv.scan.size(); ++i) {
      const SegscanChunk& c = lv.scan[i];
      if (i) CHECK(lv.scan[i - 1].len >= c.len);               // by len descending
      CHECK(c.len >= 1 && c.len <= (uint32_t)chunk);
      // every range [begin, begin +- len) lies inside [0, n)
      const bool inside = lv.reverse ? (c.begin < n && c.begin + 1 >= c.len) : (c.begin + c.len <= n);
      CHECK(inside);
      if (!inside || c.len == 0) continue;
      uint64_t acc;
      uint32_t first = 0;
      if (c.carry == kSegscanNoCarry) {
        acc = in[l][c.begin];
        first = 1;
        res[l][c.begin] = acc;
        ++res_written[l][c.begin];
      } else {
        // every carry index names a row that an earlier launch wrote: a row of the level below, which ran before
        const bool named = l + 1 < nl && c.carry < res[l + 1].size() && res_written[l + 1][c.carry] == 1;
        CHECK(named);
        if (!named) continue;
        acc = res[l + 1][c.carry];
      }
      for (uint32_t t = first; t < c.len; ++t, ++level_products) {
        const size_t at = lv.reverse ? c.begin - t : c.begin + t;
        acc = acc * in[l][at] % P;
        res[l][at] = acc;
        ++res_written[l][at];
      }
    }
    for (int w : res_written[l]) CHECK(w == 1);                // the store ranges are disjoint and cover every row once
    CHECK(level_products == rows * (lv.seg_len - 1));
    executed += level_products;
    // every level is itself a correct scan of its input
    for (size_t r = 0; r < rows; ++r) {
      uint64_t acc = 1;
      for (size_t t = 0; t < lv.seg_len; ++t) {
        const size_t at = r * lv.seg_len + (lv.reverse ? lv.seg_len - 1 - t : t);
        acc = acc * in[l][at] % P;
        CHECK(res[l][at] == acc);
      }
    }
  }
  CHECK(plan.products == executed);
  CHECK(pol::segscan_products(chunk, rows, seg_len) == executed);
  if (nl == 1) CHECK(executed == rows * (seg_len - 1));
  // never more than 2 * count plus the recursion's own count
  if (nl > 1) CHECK(executed <= 2 * count + pol::segscan_products(chunk, rows, plan.levels[1].seg_len));
}

static int print_plan() {
  size_t rows, seg_len;
  int chunk, reverse;
  if (std::scanf("%zu %zu %d %d", &rows, &seg_len, &chunk, &reverse) != 4) return 2;
  pol::SegscanPlan plan;
  pol::segscan_plan(rows, seg_len, chunk, reverse != 0, &plan);
  std::printf("levels %zu products %zu\n", plan.levels.size(), plan.products);
  for (const auto& lv : plan.levels) {
    std::printf("level %zu %zu %d %zu %zu %zu\n", lv.rows, lv.seg_len, lv.reverse ? 1 : 0, lv.up.size(), lv.totals, lv.scan.size());
    for (const auto& c : lv.up) std::printf("%llu %u %u\n", (unsigned long long)c.begin, c.len, c.dst & ~kSegsumPartial);
    for (const auto& c : lv.scan) std::printf("%llu %u %lld\n", (unsigned long long)c.begin, c.len, c.carry == kSegscanNoCarry ? -1ll : (long long)c.carry);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "plan")) return print_plan();
  // ---- plans: rows x seg_len at every level boundary of the forced chunks, both directions ----
  for (int chunk : {2, 3, 8})
    for (size_t rows : {(size_t)1, (size_t)3, (size_t)17}) {
      const size_t c = (size_t)chunk;
      for (size_t m : {(size_t)1, (size_t)2, c - 1, c, c + 1, c * c, c * c + 1, c * c * c + 1})
        for (bool rev : {false, true}) check_plan(rows, m, chunk, rev);
    }
  check_plan(5, 32, 32, false);                                  // one chain per row
  check_plan(2, 300, 8, true);
  check_plan(64, 4096, 512, false);
  // ---- levels and products ----
  CHECK(pol::segscan_levels(8, 1) == 1 && pol::segscan_levels(8, 8) == 1 && pol::segscan_levels(8, 9) == 2);
  CHECK(pol::segscan_levels(8, 72) == 2 && pol::segscan_levels(8, 73) == 3);      // 9 chunks leave 8 totals, 10 leave 9
  CHECK(pol::segscan_levels(2, 3) == 2 && pol::segscan_levels(2, 9) == 3 && pol::segscan_levels(3, 28) == 3);
  CHECK(pol::segscan_products(32, 32768, 32) == (size_t)32768 * 31);
  CHECK(pol::segscan_products(8, 1, 9) == 8 + 7 + 0);            // scan 8, one total of 7 products, a one-entry level
  CHECK(pol::segscan_products(8, 3, 65) == 3 * (64 + 8 * 7 + 7));
  // ---- the chunk rule ----
  for (int G : {2, 4, 8}) {
    const size_t chains = pol::kSegscanWavesPerSimd * pol::kSimds * (64 / (size_t)G);
    CHECK(pol::segscan_chunk(G, chains, 4096) == 4096 && pol::segscan_chunk(G, chains * 3, 100000) == 100000);   // the rows fill the chip
    CHECK(pol::segscan_chunk(G, 1, 1) == 1 && pol::segscan_chunk(G, 1, pol::kSegscanMinChunk) == (int)pol::kSegscanMinChunk);
    CHECK(pol::segscan_chunk(G, 1, 9) == (int)pol::kSegscanMinChunk);               // the floor
    CHECK(pol::segscan_chunk(G, 1, chains * 20) == 20 && pol::segscan_chunk(G, chains / 2, 4096) == 2048);
    CHECK(pol::segscan_chunk(G, chains - 1, 4096) == 2048);
    for (size_t rows : {(size_t)1, (size_t)64, (size_t)512, (size_t)32768})
      for (size_t m : {(size_t)32, (size_t)4096, (size_t)1 << 20}) {
        const size_t c = (size_t)pol::segscan_chunk(G, rows, m);
        CHECK(c >= 1 && c <= m);
        CHECK(c == m || c == pol::kSegscanMinChunk || rows * ((m + c - 1) / c) >= chains);   // below seg_len the chains fill the chip
        CHECK(pol::segscan_fits((int)c, rows, m));
      }
  }
  // ---- what a descriptor cannot address ----
  CHECK(!pol::segscan_fits(2, 1, ((size_t)1 << 32) + 2) && pol::segscan_fits(2, 1, ((size_t)1 << 32) - 2));
  CHECK(!pol::segscan_fits(2, (size_t)1 << 20, (size_t)1 << 13) && pol::segscan_fits(2, (size_t)1 << 20, (size_t)1 << 11));
  CHECK(!pol::segscan_fits(8, (size_t)1 << 40, (size_t)1 << 40));
  // ---- the forced knob (read at every call) ----
  const int dflt = pol::segscan_chunk(4, 64, 4096);
  setenv("PGPU_SEGSCAN_CHUNK", "3", 1);
  CHECK(pol::segscan_chunk(4, 64, 4096) == 3 && pol::segscan_chunk(2, (size_t)1 << 20, 5) == 3);
  setenv("PGPU_SEGSCAN_CHUNK", "100000", 1);
  CHECK(pol::segscan_chunk(4, 1, 5) == (int)pol::kSegscanForcedMax);
  setenv("PGPU_SEGSCAN_CHUNK", "1", 1);
  CHECK(pol::segscan_chunk(4, 64, 4096) == dflt);                // below 2: ignored
  unsetenv("PGPU_SEGSCAN_CHUNK");
  CHECK(pol::segscan_chunk(4, 64, 4096) == dflt);
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
