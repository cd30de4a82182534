// CPU unit test of the plan images of the aggregation calls (pailliercryptolib_amd/csrc/policy.cpp: PlanImage,
// segsum_image / spmv_image / segscan_image / wsum_image): what pgpu_batch_ct_segment_sum / _spmv / _segment_scan /
// _weighted_sum upload in one copy, and the rows of device scratch their levels rotate through.  Pure host logic -- built
// with g++ from policy.cpp alone, no device, no HIP call.  Every offset is checked against the layout written out here by
// hand ("Aggregation calls: one host driver"), every section against the vector it was made from, and the
// scratch rows of consecutive levels against each other: a level never writes a row it, or the level after it, still reads.
#include <cstdio>
#include <cstring>
#include <vector>

#include "policy.hpp"

namespace pol = pgpu::policy;
using pgpu::SegscanChunk;
using pgpu::SegsumChunk;
using pgpu::WsumSlice;
using pgpu::WsumStep;
static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      ++g_failed;                                                          \
      std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);          \
    }                                                                      \
  } while (0)

static size_t up16(size_t n) { return (n + 15) / 16 * 16; }

template <class T>
static bool section_is(const pol::PlanImage& im, size_t at, const std::vector<T>& v) {
  const size_t n = v.size() * sizeof(T);
  return at + n <= im.size() && (n == 0 || std::memcmp(im.data() + at, v.data(), n) == 0);
}
static bool zero(const pol::PlanImage& im, size_t from, size_t to) {
  for (size_t i = from; i < to; ++i)
    if (i >= im.size() || im.data()[i] != 0) return false;
  return true;
}

// Stage i of a call writes written[i] rows, from row 0 on, into region (first + i) & 1 and reads the rows stage i - 1
// wrote; region 0 starts at row 0 of the allocation, region 1 at row region[0].
static void check_rotation(const std::vector<size_t>& written, size_t first, const size_t region[2]) {
  const size_t base[2] = {0, region[0]};
  for (size_t i = 0; i < written.size(); ++i) {
    const size_t w = (first + i) & 1;
    CHECK(written[i] <= region[w]);                                   // inside its region, so inside the allocation
    if (i == 0 || written[i] == 0 || written[i - 1] == 0) continue;
    const size_t rd = (first + i - 1) & 1;
    CHECK(rd != w);
    CHECK(base[w] + written[i] <= base[rd] || base[rd] + written[i - 1] <= base[w]);   // disjoint row ranges
  }
  size_t most[2] = {0, 0};                                            // and no region larger than its largest user
  for (size_t i = 0; i < written.size(); ++i) most[(first + i) & 1] = std::max(most[(first + i) & 1], written[i]);
  CHECK(most[0] == region[0] && most[1] == region[1]);
}

static void test_builder() {
  pol::PlanImage im;
  const uint32_t a[3] = {1, 2, 3};
  const uint64_t b[2] = {4, 5};
  CHECK(im.add(a, sizeof a) == 0 && im.size() == 12);
  CHECK(im.add(b, sizeof b, 16) == 16 && im.size() == 32);           // padded up to the boundary, with zeros
  CHECK(zero(im, 12, 16));
  CHECK(im.add(nullptr, 4) == 32 && im.size() == 36 && zero(im, 32, 36));   // no source: zeros
  CHECK(im.add(a, 0, 16) == 48 && im.size() == 48);                  // an empty section still pads
  CHECK(im.add(std::vector<uint32_t>{7, 8}) == 48 && im.size() == 56);
  CHECK(std::memcmp(im.data(), a, 12) == 0 && std::memcmp(im.data() + 16, b, 16) == 0);
}

static void test_segsum(const std::vector<uint32_t>& perm, const std::vector<size_t>& offsets, int chunk, size_t want_levels) {
  pol::SegsumPlan plan;
  pol::segsum_plan(offsets, chunk, &plan);
  CHECK(plan.levels.size() == want_levels);
  pol::SegsumImage img;
  pol::segsum_image(perm, plan, &img);
  // the sorted list, at least one entry of it, padded to 16 bytes; then the descriptors of level 0, 1, ... packed
  const size_t list = perm.empty() ? 1 : perm.size();
  size_t at = up16(list * 4);
  CHECK(section_is(img.image, 0, perm));
  CHECK(zero(img.image, perm.size() * 4, at));
  CHECK(img.level_at.size() == plan.levels.size());
  std::vector<size_t> written;
  for (size_t l = 0; l < plan.levels.size(); ++l) {
    CHECK(img.level_at[l] == at && at % 16 == 0);
    CHECK(section_is(img.image, at, plan.levels[l].chunks));
    at += plan.levels[l].chunks.size() * 16;
    written.push_back(plan.levels[l].partial_rows);
  }
  CHECK(img.image.size() == at);
  check_rotation(written, 0, img.region);
}

static void test_spmv() {
  // 3 rows of 0, 1 and 5 entries at chunk 2: the long row is 3 chains, folded in two levels
  const uint64_t row_ptr[4] = {0, 0, 1, 6};
  const std::vector<uint32_t> col_idx = {4, 0, 3, 3, 1, 2};
  pol::SpmvPlan plan;
  CHECK(pol::spmv_plan(row_ptr, 3, 2, &plan));
  CHECK(plan.chains.size() == 5 && plan.partial_rows == 3 && plan.fold.levels.size() == 2);
  pol::SpmvImage img;
  pol::spmv_image(col_idx.data(), col_idx.size(), plan, &img);
  // 6 column numbers = 24 bytes, padded to 32; 5 chain descriptors; the fold levels
  CHECK(section_is(img.image, 0, col_idx) && zero(img.image, 24, 32));
  CHECK(img.chains_at == 32 && section_is(img.image, 32, plan.chains));
  size_t at = 32 + 5 * 16;
  std::vector<size_t> written = {plan.partial_rows};
  CHECK(img.fold_at.size() == plan.fold.levels.size());
  for (size_t f = 0; f < plan.fold.levels.size(); ++f) {
    CHECK(img.fold_at[f] == at);
    CHECK(section_is(img.image, at, plan.fold.levels[f].chunks));
    at += plan.fold.levels[f].chunks.size() * 16;
    written.push_back(plan.fold.levels[f].partial_rows);
  }
  CHECK(img.image.size() == at);
  CHECK(img.region[0] == 3);                                          // the chains' partial rows, more than any fold level's
  check_rotation(written, 0, img.region);
}

static void test_segscan(bool reverse) {
  // 2 rows x 5 at chunk 2: 3 chunks per row, 2 totals per row; the 2 x 2 totals are one chunk per row: 2 levels
  pol::SegscanPlan plan;
  pol::segscan_plan(2, 5, 2, reverse, &plan);
  CHECK(plan.levels.size() == 2 && plan.levels[0].totals == 4 && plan.levels[1].totals == 0);
  CHECK(plan.levels[1].rows * plan.levels[1].seg_len == plan.levels[0].totals);
  pol::SegscanImage img;
  pol::segscan_image(plan, &img);
  const size_t nl = plan.levels.size();
  CHECK(img.up_at.size() == nl && img.scan_at.size() == nl && img.totals_at.size() == nl && img.carry_at.size() == nl);
  size_t at = 0, row = 0;
  for (size_t l = 0; l < nl; ++l) {
    const auto& lv = plan.levels[l];
    CHECK(img.up_at[l] == at && section_is(img.image, at, lv.up));
    at += lv.up.size() * 16;
    CHECK(img.scan_at[l] == at && section_is(img.image, at, lv.scan));
    at += lv.scan.size() * 16;
    // the level's totals, then as many carries: level l + 1 reads the former and writes the latter
    CHECK(img.totals_at[l] == row && img.carry_at[l] == row + lv.totals);
    row += 2 * lv.totals;
  }
  CHECK(img.image.size() == at && img.scratch_rows == row && row == 8);
  // every range of totals and of carries is a range of its own
  std::vector<std::pair<size_t, size_t>> ranges;
  for (size_t l = 0; l < nl; ++l) {
    ranges.push_back({img.totals_at[l], img.totals_at[l] + plan.levels[l].totals});
    ranges.push_back({img.carry_at[l], img.carry_at[l] + plan.levels[l].totals});
  }
  for (size_t i = 0; i < ranges.size(); ++i) {
    CHECK(ranges[i].second <= img.scratch_rows);
    for (size_t j = 0; j < i; ++j)
      CHECK(ranges[i].first == ranges[i].second || ranges[j].first == ranges[j].second ||
            ranges[i].second <= ranges[j].first || ranges[j].second <= ranges[i].first);
  }
}

static void test_wsum(size_t S) {
  const uint64_t weights[3] = {5, 3, 6};
  pol::WsumPlan plan, fold;
  CHECK(pol::wsum_plan(weights, 1, 3, S, &plan));
  CHECK(plan.slices.size() == S);
  if (S > 1) CHECK(pol::wsum_plan(nullptr, 0, S, 1, &fold));
  CHECK(fold.slices.size() == (S > 1 ? 1u : 0u));
  static uint32_t rows[5][4];                                         // stand-ins for the batches' row bases
  std::vector<const uint32_t*> tab = {rows[0], rows[1], rows[2]}, ftab;
  for (size_t j = 0; j < S; ++j) plan.slices[j].dst = rows[3 + (j > 0)];
  if (S > 1) {
    for (size_t j = 0; j < S; ++j) ftab.push_back(plan.slices[j].dst);
    fold.slices[0].dst = rows[3];
  }
  pol::WsumImage img;
  pol::wsum_image(tab, ftab, plan, fold, &img);
  // row bases of the terms, of the slices (with a fold only), the slices, the fold's slice, the steps, the fold's steps
  const size_t P = sizeof(uint32_t*), SL = sizeof(WsumSlice), ST = sizeof(WsumStep);
  CHECK(SL == 40 && ST == 8);
  CHECK(img.tab_at == 0 && section_is(img.image, 0, tab));
  CHECK(img.ftab_at == 3 * P && section_is(img.image, img.ftab_at, ftab));
  CHECK(img.slices_at == 3 * P + (S > 1 ? S : 0) * P && section_is(img.image, img.slices_at, plan.slices));
  CHECK(img.fold_slices_at == img.slices_at + S * SL && section_is(img.image, img.fold_slices_at, fold.slices));
  CHECK(img.steps_at == img.fold_slices_at + (S > 1 ? 1 : 0) * SL && section_is(img.image, img.steps_at, plan.steps));
  CHECK(img.fold_steps_at == img.steps_at + plan.steps.size() * ST && section_is(img.image, img.fold_steps_at, fold.steps));
  CHECK(img.image.size() == img.fold_steps_at + fold.steps.size() * ST);
}

int main() {
  test_builder();
  // 7 elements in 3 segments of 4, 2 and 1 at chunk 2: two levels, the first leaves two partial rows
  test_segsum({3, 0, 6, 1, 5, 2, 4}, {0, 4, 6, 7}, 2, 2);
  // 9 in one segment at chunk 2: four levels, both regions used twice
  test_segsum({0, 1, 2, 3, 4, 5, 6, 7, 8}, {0, 9}, 2, 4);
  // nothing selected: an empty sorted list still leaves one (zero) entry for the kernel to read
  test_segsum({}, {0, 0, 0, 0}, 2, 1);
  test_spmv();
  test_segscan(false);
  test_segscan(true);
  test_wsum(1);
  test_wsum(2);
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
