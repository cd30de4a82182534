// CPU unit test of the host side of gather / concat / slice of resident batches (pailliercryptolib_amd/csrc/policy.cpp:
// gather_plan / gather_descs / gather_slice_descs / gather_image): row size -> launch shape, flat index -> (source, row)
// across ragged sources, the first out-of-range position, the sentinel, the sections of the plan image.  Pure host logic --
// built with g++ from policy.cpp alone, no device, no HIP call; tests/test_gather_policy.py also builds it with
// -fsanitize=address,undefined and runs it as a plain program.  In the reference the re-ordering calls
// (CipherText::rotate / getChunk / getCipherText, ipcl/ciphertext.cpp, base_text.cpp) index host vectors; the rules here are
// documented in DESIGN.md ("Gather, concat and slice of resident batches").
#include <cstdio>
#include <cstring>
#include <vector>

#include "policy.hpp"

namespace pol = pgpu::policy;
using pgpu::GatherDesc;
using pgpu::kGatherOneRow;
static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      ++g_failed;                                                          \
      std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);          \
    }                                                                      \
  } while (0)

static void test_plan() {
  // row bytes -> (piece bytes, lanes per row, rows per wavefront): rows of 8 bytes are one piece; 16-byte pieces only
  // where the row is a multiple of 16; at most 16 lanes per row, so at least 4 rows per wavefront
  struct { size_t row; int vec, lanes, rows; } want[] = {
      {8, 8, 1, 64},      // words = 1: plaintext / randomness batches
      {16, 16, 1, 64},    {24, 8, 4, 16},    // words = 3: three 8-byte pieces
      {32, 16, 2, 32},    {256, 16, 16, 4},
      {264, 8, 16, 4},    // words = 33: 33 pieces of 8, three sweeps of 16 lanes
      {304, 16, 16, 4},   // pair rows of a 1024-bit key: 19 pieces
      {576, 16, 16, 4},   // ... of a 2048-bit key: 36 pieces
      {896, 16, 16, 4},   // ... of a 3072-bit key: 56 pieces
      {1024, 16, 16, 4},
  };
  for (const auto& w : want) {
    pol::GatherPlan p;
    CHECK(pol::gather_plan(w.row, 1000, &p));
    CHECK(p.vec_bytes == w.vec && p.lanes_per_row == w.lanes && p.rows_per_wavefront == w.rows);
    CHECK(p.lanes_per_row == 1 << p.lanes_log2 && p.lanes_per_row * p.rows_per_wavefront == 64);
    CHECK(p.lanes_per_row <= pgpu::kGatherMaxLanes && p.rows_per_wavefront >= 4);
    CHECK((p.vec_bytes == 16) == (w.row % 16 == 0));
    CHECK(w.row % (size_t)p.vec_bytes == 0);
    // never one lane per multi-piece row
    CHECK(p.lanes_per_row > 1 || w.row / (size_t)p.vec_bytes == 1);
    CHECK(p.wavefronts == (1000 + (size_t)w.rows - 1) / (size_t)w.rows && p.blocks == (p.wavefronts + 3) / 4);
  }
  for (size_t row = 8; row <= 4096; row += 8) {   // every width: the 16-byte form only for multiples of 16
    pol::GatherPlan p;
    CHECK(pol::gather_plan(row, 1, &p));
    CHECK((p.vec_bytes == 16) == (row % 16 == 0) && (p.vec_bytes == 16 || p.vec_bytes == 8));
    CHECK(p.wavefronts == 1 && p.blocks == 1);
  }
  pol::GatherPlan p;
  p.vec_bytes = -1;
  CHECK(!pol::gather_plan(0, 10, &p) && !pol::gather_plan(12, 10, &p) && !pol::gather_plan(576, 0, &p) && p.vec_bytes == -1);
  // the wavefront count at the edges of a wavefront and of a workgroup
  CHECK(pol::gather_plan(576, 4, &p) && p.wavefronts == 1 && p.blocks == 1);
  CHECK(pol::gather_plan(576, 5, &p) && p.wavefronts == 2 && p.blocks == 1);
  CHECK(pol::gather_plan(576, 17, &p) && p.wavefronts == 5 && p.blocks == 2);
}

static void test_descs() {
  // ragged sources, one of them named twice (to the translation: two stretches of the concatenation)
  const size_t counts[] = {3, 1, 5, 3, 2};   // total 14; starts 0 3 4 9 12
  const size_t starts[] = {0, 3, 4, 9, 12};
  std::vector<uint64_t> idx;
  for (uint64_t v = 0; v < 14; ++v) idx.push_back(v);
  std::vector<GatherDesc> d;
  CHECK(pol::gather_descs(counts, 5, idx.data(), idx.size(), &d) == 14 && d.size() == 14);
  for (size_t v = 0; v < 14; ++v) {
    size_t k = 0;
    while (k + 1 < 5 && v >= starts[k + 1]) ++k;
    CHECK(d[v].source == k && d[v].row == v - starts[k]);
  }
  // any order, repeats, the sentinel at both ends and in between
  const uint64_t mix[] = {pol::kGatherOne, 13, 0, 13, 4, 3, 8, pol::kGatherOne, 9, 2, 12, 0, pol::kGatherOne};
  CHECK(pol::gather_descs(counts, 5, mix, 13, &d) == 13);
  const GatherDesc want[] = {{0, kGatherOneRow}, {4, 1}, {0, 0}, {4, 1}, {2, 0}, {1, 0}, {2, 4}, {0, kGatherOneRow}, {3, 0},
                             {0, 2}, {4, 0}, {0, 0}, {0, kGatherOneRow}};
  for (size_t i = 0; i < 13; ++i) CHECK(d[i].source == want[i].source && d[i].row == want[i].row);
  // the first out-of-range position
  const uint64_t bad[] = {1, 2, 14, 0, 99};
  CHECK(pol::gather_descs(counts, 5, bad, 5, &d) == 2);
  const uint64_t bad0[] = {~(uint64_t)0 - 1, 0};
  CHECK(pol::gather_descs(counts, 5, bad0, 2, &d) == 0);
  const uint64_t bad_last[] = {pol::kGatherOne, 13, 14};
  CHECK(pol::gather_descs(counts, 5, bad_last, 3, &d) == 2);
  // one source; 300 sources of one row each
  const size_t one[] = {7};
  const uint64_t rev[] = {6, 5, 4, 3, 2, 1, 0};
  CHECK(pol::gather_descs(one, 1, rev, 7, &d) == 7);
  for (size_t i = 0; i < 7; ++i) CHECK(d[i].source == 0 && d[i].row == 6 - i);
  std::vector<size_t> many(300, 1);
  idx.clear();
  for (uint64_t v = 0; v < 300; ++v) idx.push_back(299 - v);
  CHECK(pol::gather_descs(many.data(), 300, idx.data(), 300, &d) == 300);
  for (size_t i = 0; i < 300; ++i) CHECK(d[i].source == 299 - i && d[i].row == 0);
  // a source of 2^32 - 2 rows: the largest row number stays below the sentinel
  const size_t big[] = {2, pol::kGatherMaxRows - 1};
  const uint64_t last[] = {pol::kGatherMaxRows, 1, 2};
  CHECK(pol::gather_descs(big, 2, last, 3, &d) == 3);
  CHECK(d[0].source == 1 && d[0].row == 0xFFFFFFFDu && d[0].row < kGatherOneRow && d[1].source == 0 && d[2].source == 1 && d[2].row == 0);
  // ... and that is the largest source the calls admit: 2^32 - 1 rows or more are refused, the first such source named
  CHECK(pol::gather_counts_ok(big, 2) == 2);
  const size_t too_big[] = {5, pol::kGatherMaxRows - 1, pol::kGatherMaxRows, (size_t)1 << 40};
  CHECK(pol::gather_counts_ok(too_big, 4) == 2 && pol::gather_counts_ok(too_big, 2) == 2 && pol::gather_counts_ok(too_big + 3, 1) == 0);
  CHECK(pol::gather_counts_ok(too_big, 0) == 0);
  // the strided slice
  pol::gather_slice_descs(3, 4, 7, &d);
  CHECK(d.size() == 4);
  for (size_t i = 0; i < 4; ++i) CHECK(d[i].source == 0 && d[i].row == 3 + 7 * i);
}

static void test_image() {
  for (size_t row_bytes : {(size_t)8, (size_t)24, (size_t)576}) {
    for (size_t n_src : {(size_t)1, (size_t)2, (size_t)3}) {
      std::vector<const char*> bases;
      for (size_t k = 0; k < n_src; ++k) bases.push_back((const char*)(uintptr_t)(0x1000 * (k + 1)));
      std::vector<char> one(row_bytes, 0);
      for (size_t i = 0; i < row_bytes; ++i) one[i] = (char)(i + 1);
      std::vector<GatherDesc> d = {{0, 5}, {(uint32_t)(n_src - 1), kGatherOneRow}, {0, 0}};
      pol::GatherImage img;
      pol::gather_image(bases, one.data(), row_bytes, d, &img);
      CHECK(img.bases_at == 0);
      CHECK(img.one_at % 16 == 0 && img.one_at >= n_src * 8 && img.one_at < n_src * 8 + 16);
      CHECK(img.desc_at % 8 == 0 && img.desc_at >= img.one_at + row_bytes && img.desc_at < img.one_at + row_bytes + 8);
      CHECK(img.image.size() == img.desc_at + d.size() * sizeof(GatherDesc));
      CHECK(std::memcmp(img.image.data() + img.bases_at, bases.data(), n_src * 8) == 0);
      CHECK(std::memcmp(img.image.data() + img.one_at, one.data(), row_bytes) == 0);
      CHECK(std::memcmp(img.image.data() + img.desc_at, d.data(), d.size() * sizeof(GatherDesc)) == 0);
    }
  }
  // 40000 descriptors: beyond a 256 KiB bounce buffer
  std::vector<GatherDesc> d(40000, GatherDesc{0, 1});
  std::vector<char> one(304, 0);
  pol::GatherImage img;
  pol::gather_image({nullptr}, one.data(), 304, d, &img);
  CHECK(img.image.size() == 16 + 304 + 40000 * 8 && img.image.size() > ((size_t)256 << 10));
}

int main() {
  test_plan();
  test_descs();
  test_image();
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
