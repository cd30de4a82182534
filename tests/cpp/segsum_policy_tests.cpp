// CPU unit test of the plan of the encrypted segmented sum (pailliercryptolib_amd/csrc/policy.cpp: segsum_*): the stable
// counting sort of the element numbers by segment id, the chunk rule, the level count and the chunk descriptors of every
// level.  Pure host logic -- built with g++ from policy.cpp alone, no device, no HIP call.  In the reference such a sum is
// composed from CipherText::operator+ (ipcl/ciphertext.cpp:35-72) after a gather on the host; the rule is documented in
// DESIGN.md ("Encrypted segmented sum").
//
// `segsum_policy_tests plan` reads "groups cols n_segments chunk" and groups*cols ids from standard input and prints the
// plan (tests/test_segsum_model.py replays it in plain integers).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <random>
#include <vector>

#include "policy.hpp"

namespace pol = pgpu::policy;
using pgpu::kSegsumPartial;
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

static const uint32_t NONE = pol::kSegsumNone;

// Replays a plan on index SETS: every level must tile its input lists exactly once, route the last chunk of a segment to
// the segment's output row and everything else to a fresh partial row, keep the len-descending order, and end with one
// row per segment that holds exactly the entries of perm in that segment's range.
static void check_plan(const std::vector<size_t>& offsets, int chunk) {
  pol::SegsumPlan plan;
  pol::segsum_plan(offsets, chunk, &plan);
  const size_t segments = offsets.size() - 1;
  size_t longest = 0;
  for (size_t s = 0; s < segments; ++s) longest = std::max(longest, offsets[s + 1] - offsets[s]);
  CHECK(plan.chunk == chunk && plan.longest == longest);
  CHECK((int)plan.levels.size() == pol::segsum_levels(chunk, longest));
  CHECK(plan.levels.size() >= 1);
  // a row = the sorted list of perm positions it is the product of
  std::vector<std::vector<size_t>> out(segments), prev, cur;
  std::vector<int> written(segments, 0);
  for (size_t l = 0; l < plan.levels.size(); ++l) {
    const auto& lv = plan.levels[l];
    cur.assign(lv.partial_rows, {});
    std::vector<int> cur_written(lv.partial_rows, 0);
    const size_t n_in = l == 0 ? offsets[segments] : prev.size();
    std::vector<int> used(n_in, 0);
    for (size_t i = 0; i < lv.chunks.size(); ++i) {
      const SegsumChunk& c = lv.chunks[i];
      if (i) CHECK(lv.chunks[i - 1].len >= c.len);
      CHECK(c.len <= (uint32_t)chunk);
      CHECK(c.begin + c.len <= n_in);
      std::vector<size_t> row;
      for (uint32_t t = 0; t < c.len && c.begin + t < n_in; ++t) {
        ++used[c.begin + t];
        if (l == 0) row.push_back(c.begin + t);
        else row.insert(row.end(), prev[c.begin + t].begin(), prev[c.begin + t].end());
      }
      if (c.dst & kSegsumPartial) {
        const size_t r = c.dst & ~kSegsumPartial;
        CHECK(r < lv.partial_rows);
        if (r < lv.partial_rows) { ++cur_written[r]; cur[r] = row; }
        CHECK(c.len >= 1);
      } else {
        CHECK(c.dst < segments);
        if (c.dst < segments) { ++written[c.dst]; out[c.dst] = row; }
      }
    }
    for (int u : used) CHECK(u == 1);                 // the chunks tile the input exactly once
    for (int w : cur_written) CHECK(w == 1);
    if (l + 1 == plan.levels.size()) CHECK(lv.partial_rows == 0);
    prev.swap(cur);
  }
  for (size_t s = 0; s < segments; ++s) {
    CHECK(written[s] == 1);                            // one row per segment, written once, by its last level
    CHECK(out[s].size() == offsets[s + 1] - offsets[s]);
    for (size_t k = 0; k < out[s].size(); ++k) CHECK(out[s][k] == offsets[s] + k);
  }
}

static int print_plan() {
  size_t groups, cols, n_segments;
  int chunk;
  if (std::scanf("%zu %zu %zu %d", &groups, &cols, &n_segments, &chunk) != 4) return 2;
  std::vector<uint32_t> ids(groups * cols);
  for (auto& v : ids) if (std::scanf("%u", &v) != 1) return 2;
  std::vector<uint32_t> perm;
  std::vector<size_t> offsets;
  if (!pol::segsum_sort(ids.data(), groups, cols, n_segments, &perm, &offsets)) { std::printf("bad id\n"); return 3; }
  pol::SegsumPlan plan;
  pol::segsum_plan(offsets, chunk, &plan);
  std::printf("perm");
  for (uint32_t v : perm) std::printf(" %u", v);
  std::printf("\nlevels %zu\n", plan.levels.size());
  for (const auto& lv : plan.levels) {
    std::printf("level %zu %zu\n", lv.chunks.size(), lv.partial_rows);
    for (const auto& c : lv.chunks)
      std::printf("%llu %u %u %u\n", (unsigned long long)c.begin, c.len, c.dst & ~kSegsumPartial, (c.dst & kSegsumPartial) ? 1u : 0u);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "plan")) return print_plan();
  std::vector<uint32_t> perm;
  std::vector<size_t> off;
  // ---- the counting sort: stable, NONE dropped, out-of-range refused ----
  {
    const uint32_t ids[] = {2, 0, NONE, 2, 1, 0, 2, NONE};
    CHECK(pol::segsum_sort(ids, 1, 8, 3, &perm, &off));
    CHECK((perm == std::vector<uint32_t>{1, 5, 4, 0, 3, 6}));
    CHECK((off == std::vector<size_t>{0, 2, 3, 6}));
    CHECK(pol::segsum_sort(ids, 2, 4, 3, &perm, &off));          // the same ids as two groups of four elements
    CHECK((perm == std::vector<uint32_t>{1, 0, 3, 1, 0, 2}));    // element numbers restart in every group
    CHECK((off == std::vector<size_t>{0, 1, 1, 3, 4, 5, 6}));
    perm = {77};
    off = {9};
    CHECK(!pol::segsum_sort(ids, 1, 8, 2, &perm, &off));         // id 2 with two segments
    CHECK(perm == std::vector<uint32_t>{77} && off == std::vector<size_t>{9});   // nothing written on a refusal
    const uint32_t big[] = {0, 0xFFFFFFFEu};
    CHECK(!pol::segsum_sort(big, 1, 2, 5, &perm, &off));
    const uint32_t none[] = {NONE, NONE, NONE};
    CHECK(pol::segsum_sort(none, 1, 3, 2, &perm, &off) && perm.empty() && (off == std::vector<size_t>{0, 0, 0}));
    CHECK(pol::segsum_sort(none, 3, 0, 2, &perm, &off) && perm.empty() && off.size() == 7);   // no elements at all
  }
  // ---- levels: ceil(log_chunk(longest)), at least 1 ----
  CHECK(pol::segsum_levels(8, 0) == 1 && pol::segsum_levels(8, 1) == 1 && pol::segsum_levels(8, 8) == 1);
  CHECK(pol::segsum_levels(8, 9) == 2 && pol::segsum_levels(8, 64) == 2 && pol::segsum_levels(8, 65) == 3);
  CHECK(pol::segsum_levels(2, 37) == 6 && pol::segsum_levels(2, 32) == 5 && pol::segsum_levels(2, 33) == 6);
  CHECK(pol::segsum_levels(3, 10) == 3 && pol::segsum_levels(64, 4097) == 3 && pol::segsum_levels(64, 4096) == 2);
  CHECK(pol::segsum_levels(256, (size_t)1 << 20) == 3);
  // ---- the chunk rule: fill the chip at level 0, between the two bounds ----
  CHECK(pol::kSegsumMinChunk >= 2 && pol::kSegsumMinChunk <= pol::kSegsumMaxChunk);
  for (int G : {2, 4, 8}) {
    const size_t chains = pol::kSegsumWavesPerSimd * pol::kSimds * (64 / (size_t)G);
    CHECK(pol::segsum_chunk(G, 0) == (int)pol::kSegsumMinChunk && pol::segsum_chunk(G, 1) == (int)pol::kSegsumMinChunk);
    CHECK(pol::segsum_chunk(G, chains * pol::kSegsumMinChunk) == (int)pol::kSegsumMinChunk);
    CHECK(pol::segsum_chunk(G, chains * 20) == (int)std::max<size_t>(20, pol::kSegsumMinChunk));
    CHECK(pol::segsum_chunk(G, chains * 20 + chains - 1) == (int)std::max<size_t>(20, pol::kSegsumMinChunk));
    CHECK(pol::segsum_chunk(G, chains * pol::kSegsumMaxChunk * 4) == (int)pol::kSegsumMaxChunk);
    for (size_t e : {(size_t)1 << 16, (size_t)1 << 20, (size_t)1 << 24}) {
      const size_t c = (size_t)pol::segsum_chunk(G, e);
      CHECK(c >= pol::kSegsumMinChunk && c <= pol::kSegsumMaxChunk);
      CHECK(c == pol::kSegsumMinChunk || e / c >= chains);      // above the lower bound the level-0 chains fill the chip
    }
  }
  // ---- the wide form: levels that leave SIMDs empty at 64/wide_G chains per wavefront ----
  CHECK(pol::segsum_wide_pays(8, 0) && pol::segsum_wide_pays(8, 1) && pol::segsum_wide_pays(8, 8 * pol::kSimds));
  CHECK(!pol::segsum_wide_pays(8, 8 * pol::kSimds + 1) && !pol::segsum_wide_pays(8, (size_t)1 << 20));
  CHECK(pol::segsum_wide_pays(16, 4 * pol::kSimds) && !pol::segsum_wide_pays(16, 4 * pol::kSimds + 1));
  // ---- plans: shapes of the GPU tests and the edges, at the chunks the tests force ----
  std::mt19937 rng(7);
  for (int chunk : {2, 3, 8, 64}) {
    check_plan({0, 0}, chunk);                                     // one empty segment
    check_plan({0, 0, 0, 0}, chunk);
    check_plan({0, 1}, chunk);
    check_plan({0, (size_t)chunk}, chunk);
    check_plan({0, (size_t)chunk + 1}, chunk);
    check_plan({0, (size_t)chunk * chunk}, chunk);
    check_plan({0, (size_t)chunk * chunk + 1}, chunk);
    check_plan({0, 37, 37, 38, 300}, chunk);
    for (int it = 0; it < 20; ++it) {
      std::vector<size_t> o{0};
      const int segs = 1 + rng() % 12;
      for (int s = 0; s < segs; ++s) o.push_back(o.back() + (rng() % 4 == 0 ? 0 : rng() % (it % 2 ? 40 : 700)));
      check_plan(o, chunk);
    }
  }
  {
    pol::SegsumPlan p;
    pol::segsum_plan({0, 37, 37}, 2, &p);                          // chunk 2 on 37 elements: 19, 10, 5, 3, 2, 1 rows
    CHECK(p.levels.size() == 6 && p.levels[0].partial_rows == 19 && p.levels[4].partial_rows == 2);
    CHECK(p.levels[0].chunks.size() == 20 && p.levels[0].chunks.back().len == 0 && p.levels[0].chunks.back().dst == 1);
    CHECK(p.levels[5].chunks.size() == 1 && p.levels[5].chunks[0].dst == 0 && p.levels[5].chunks[0].len == 2);
    pol::segsum_plan({0, 5, 9}, 8, &p);                            // short segments: one level, straight into the result
    CHECK(p.levels.size() == 1 && p.levels[0].partial_rows == 0 && p.levels[0].chunks[0].len == 5 && p.levels[0].chunks[1].dst == 1);
  }
  // ---- the forced knob (read at every call) ----
  const int dflt = pol::segsum_chunk(4, (size_t)1 << 20);
  setenv("PGPU_SEGSUM_CHUNK", "3", 1);
  CHECK(pol::segsum_chunk(4, (size_t)1 << 20) == 3 && pol::segsum_chunk(2, 0) == 3);
  setenv("PGPU_SEGSUM_CHUNK", "1000", 1);
  CHECK(pol::segsum_chunk(4, 5) == 1000);                           // beyond the upper bound of the rule: honoured
  setenv("PGPU_SEGSUM_CHUNK", "100000", 1);
  CHECK(pol::segsum_chunk(4, 5) == (int)pol::kSegsumForcedMax);     // ... up to the cap
  setenv("PGPU_SEGSUM_CHUNK", "1", 1);
  CHECK(pol::segsum_chunk(4, (size_t)1 << 20) == dflt);             // below 2: ignored
  unsetenv("PGPU_SEGSUM_CHUNK");
  CHECK(pol::segsum_chunk(4, (size_t)1 << 20) == dflt);
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
