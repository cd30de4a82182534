// CPU unit test of the plan of the encrypted sparse matrix-vector product (pailliercryptolib_amd/csrc/policy.cpp: spmv_*):
// (nnz, rows) -> chunk, row_ptr -> chain descriptors and fold levels, totals -> window and product count.  Pure host logic
// -- built with g++ from policy.cpp alone, no device, no HIP call.  With the argument "plan" the binary reads
// "rows chunk" and rows + 1 offsets from stdin and prints the plan (tests/test_spmv_model.py walks it in integers).  In
// the reference such a map is composed from CipherText::operator* (ipcl/ciphertext.cpp:83-106) and operator+
// (ciphertext.cpp:35-72) term by term; the rule is documented in DESIGN.md ("Encrypted sparse matrix-vector product").
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
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

static int print_plan() {
  size_t rows = 0;
  int chunk = 0;
  if (std::scanf("%zu %d", &rows, &chunk) != 2) return 2;
  std::vector<uint64_t> rp(rows + 1);
  for (auto& v : rp)
    if (std::scanf("%lu", &v) != 1) return 2;
  pol::SpmvPlan plan;
  if (!pol::spmv_plan(rp.data(), rows, chunk, &plan)) {
    std::printf("refused\n");
    return 0;
  }
  std::printf("chains %zu %zu %zu\n", plan.chains.size(), plan.partial_rows, plan.longest);
  for (const SegsumChunk& k : plan.chains)
    std::printf("%lu %u %u %d\n", (unsigned long)k.begin, k.len, k.dst & ~kSegsumPartial, (k.dst & kSegsumPartial) ? 1 : 0);
  std::printf("fold %zu %d\n", plan.fold.levels.size(), plan.fold.chunk);
  for (const auto& lv : plan.fold.levels) {
    std::printf("level %zu %zu\n", lv.chunks.size(), lv.partial_rows);
    for (const SegsumChunk& k : lv.chunks)
      std::printf("%lu %u %u %d\n", (unsigned long)k.begin, k.len, k.dst & ~kSegsumPartial, (k.dst & kSegsumPartial) ? 1 : 0);
  }
  return 0;
}

// the descriptors of a plan against the matrix they were made for
static void check_plan(const std::vector<uint64_t>& rp, int chunk) {
  const size_t rows = rp.size() - 1, nnz = (size_t)rp[rows], c = (size_t)chunk;
  pol::SpmvPlan plan;
  CHECK(pol::spmv_plan(rp.data(), rows, chunk, &plan));
  CHECK(plan.chunk == chunk && plan.n_chains == plan.chains.size());
  // every CSR position lies in exactly one chain, which belongs to the row of that position; every row has its chains
  std::vector<int> seen(nnz, 0);
  std::vector<size_t> chains_of(rows, 0), partial_owner(plan.partial_rows, (size_t)-1);
  size_t want_chains = 0, want_partial = 0, longest = 0, empty_rows = 0, empty_chains = 0;
  for (size_t i = 0; i < rows; ++i) {
    const size_t m = (size_t)(rp[i + 1] - rp[i]), parts = m <= c ? 1 : (m + c - 1) / c;
    want_chains += parts;
    if (parts > 1) want_partial += parts;
    longest = m > longest ? m : longest;
    empty_rows += m == 0;
  }
  CHECK(plan.chains.size() == want_chains && plan.partial_rows == want_partial && plan.longest == longest);
  for (size_t k = 0; k < plan.chains.size(); ++k) {
    const SegsumChunk& d = plan.chains[k];
    CHECK(d.len <= c && d.begin + d.len <= nnz);
    if (k) CHECK(plan.chains[k - 1].len >= d.len);                 // ordered by length
    empty_chains += d.len == 0;
    // the row of the chain: the one whose range holds begin (an empty chain names its row directly)
    size_t row = 0;
    if (d.dst & kSegsumPartial) {
      const size_t pr = d.dst & ~kSegsumPartial;
      CHECK(pr < plan.partial_rows && d.len >= 1);
      while (row < rows && !(rp[row] <= d.begin && d.begin < rp[row + 1])) ++row;
      CHECK(row < rows);
      if (row < rows && pr < plan.partial_rows) {
        CHECK(partial_owner[pr] == (size_t)-1);                    // a partial row is written once
        partial_owner[pr] = row;
      }
    } else {
      row = d.dst;
      CHECK(row < rows && d.begin == rp[row] && d.len == rp[row + 1] - rp[row]);   // the whole row in one chain
    }
    if (row < rows) {
      ++chains_of[row];
      CHECK(d.begin >= rp[row] && d.begin + d.len <= rp[row + 1]);
    }
    for (size_t t = 0; t < d.len && d.begin + t < nnz; ++t) ++seen[d.begin + t];
  }
  for (size_t t = 0; t < nnz; ++t) CHECK(seen[t] == 1);
  CHECK(empty_chains == empty_rows);
  for (size_t i = 0; i < rows; ++i) {
    const size_t m = (size_t)(rp[i + 1] - rp[i]);
    CHECK(chains_of[i] == (m <= c ? 1 : (m + c - 1) / c));
  }
  // the partial rows of one row are consecutive, in CSR order: what the fold's level 0 reads as one segment
  for (size_t pr = 1; pr < plan.partial_rows; ++pr) CHECK(partial_owner[pr - 1] <= partial_owner[pr]);
  // fold levels: those of a segmented sum over the partial rows -- every partial row of a level is read exactly once by the
  // next, every row of several chains is written exactly once by a descriptor without the partial flag, no other row is
  const int fc = chunk < 2 ? 2 : chunk;
  CHECK(plan.fold.levels.empty() == (plan.partial_rows == 0));
  CHECK((int)plan.fold.levels.size() + 1 == pol::spmv_levels(chunk, longest));
  std::vector<int> written(rows, 0);
  size_t in_rows = plan.partial_rows;
  std::vector<size_t> owner = partial_owner;
  for (const auto& lv : plan.fold.levels) {
    std::vector<int> read(in_rows, 0);
    std::vector<size_t> next_owner(lv.partial_rows, (size_t)-1);
    for (size_t k = 0; k < lv.chunks.size(); ++k) {
      const SegsumChunk& d = lv.chunks[k];
      CHECK(d.len >= 1 && d.len <= (size_t)fc && d.begin + d.len <= in_rows);
      if (k) CHECK(lv.chunks[k - 1].len >= d.len);
      for (size_t t = 0; t < d.len && d.begin + t < in_rows; ++t) {
        ++read[d.begin + t];
        CHECK(owner[d.begin + t] == owner[d.begin]);               // one chain folds rows of one output row
      }
      if (d.dst & kSegsumPartial) {
        const size_t pr = d.dst & ~kSegsumPartial;
        CHECK(pr < lv.partial_rows);
        if (pr < lv.partial_rows) next_owner[pr] = owner[d.begin];
      } else {
        CHECK(d.dst < rows && d.dst == owner[d.begin]);
        if (d.dst < rows) ++written[d.dst];
      }
    }
    for (size_t r = 0; r < in_rows; ++r) CHECK(read[r] == 1);
    in_rows = lv.partial_rows;
    owner.swap(next_owner);
  }
  CHECK(in_rows == 0);
  for (size_t i = 0; i < rows; ++i) CHECK(written[i] == (chains_of[i] > 1 ? 1 : 0));
}

static int best_window(size_t rows, size_t cols, size_t nnz, size_t chains, int e_bits, size_t row_bytes) {
  int best = 1;
  for (int w = 2; w <= 6; ++w)
    if (cols * ((size_t)1 << w) * row_bytes <= pol::kMatvecTableCap &&
        pol::spmv_products(rows, cols, nnz, chains, e_bits, w) < pol::spmv_products(rows, cols, nnz, chains, e_bits, best))
      best = w;
  return best;
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "plan")) return print_plan();
  // ---- chunk: the fill segsum_chunk aims at, between the floor of section 11 and the ceiling of section 12 ----
  CHECK(pol::kSpmvMinChunk == pol::kMatvecMinSliceCols && pol::kSpmvMaxChunk == pol::kSegsumMaxChunk);
  CHECK(pol::spmv_chunk(4, 1, 1) == 4 && pol::spmv_chunk(4, 1000, 10) == 4);           // the floor
  CHECK(pol::spmv_chunk(4, (size_t)1 << 20, 65536) == 8);                               // 2^20 / (8 * 1024 * 16)
  CHECK(pol::spmv_chunk(2, (size_t)1 << 20, 1024) == 4 && pol::spmv_chunk(8, (size_t)1 << 20, 1024) == 16);
  CHECK(pol::spmv_chunk(4, (size_t)1 << 26, 1) == 256 && pol::spmv_chunk(8, (size_t)1 << 30, 1) == 256);   // the ceiling
  for (int G : {2, 4, 8})
    for (size_t nnz : {(size_t)1, (size_t)600, (size_t)1 << 16, (size_t)1 << 20, (size_t)1 << 24, (size_t)1 << 30}) {
      const int c = pol::spmv_chunk(G, nnz, 1);
      CHECK(c >= (int)pol::kSpmvMinChunk && c <= (int)pol::kSpmvMaxChunk);
      CHECK(c == (int)pol::kSpmvMinChunk || c == (int)pol::kSpmvMaxChunk || (size_t)c == nnz / (8 * 1024 * (64 / (size_t)G)));
    }
  // ---- levels ----
  CHECK(pol::spmv_levels(4, 0) == 1 && pol::spmv_levels(4, 4) == 1 && pol::spmv_levels(4, 5) == 2);
  CHECK(pol::spmv_levels(4, 16) == 2 && pol::spmv_levels(4, 17) == 3);                  // 5 partial rows > 4: two fold levels
  CHECK(pol::spmv_levels(2, 20) == 5);                                                  // 10 -> 5 -> 3 -> 2 -> 1
  CHECK(pol::spmv_levels(1, 20) == 6);                                                  // 20 chains, folded by 2
  CHECK(pol::spmv_levels(256, (size_t)1 << 20) == 3);
  // ---- descriptors ----
  const std::vector<uint64_t> ragged = {0, 0, 1, 3, 6, 13, 53, 53, 54, 94, 94};         // rows of 0 1 2 3 7 40 0 1 40 0
  for (int chunk : {1, 2, 3, 4, 7, 8, 39, 40, 41, 64}) check_plan(ragged, chunk);
  check_plan({0, 5}, 4);                                                                // chunk + 1
  check_plan({0, 4}, 4);                                                                // chunk
  check_plan({0, 1}, 4);
  check_plan({0, 0, 0, 1}, 4);                                                          // leading empty rows
  check_plan({0, 1, 1, 1}, 1);
  {
    std::vector<uint64_t> rp(1, 0);                                                     // 300 rows, lengths cycling 0..16
    for (size_t i = 0; i < 300; ++i) rp.push_back(rp.back() + (i * 7) % 17);
    for (int chunk : {1, 2, 4, 5, 16, 17}) check_plan(rp, chunk);
    std::vector<uint64_t> one = {0, 100000};                                            // one very long row
    for (int chunk : {2, 256, 65536}) check_plan(one, chunk);
  }
  {
    // what the fold is: segsum_plan over the partial rows, with the output rows named
    pol::SpmvPlan plan;
    const std::vector<uint64_t> rp = {0, 2, 12, 13, 18};                                // chunk 4: rows 1 (3 chains) and 3 (2 chains) fold
    CHECK(pol::spmv_plan(rp.data(), 4, 4, &plan));
    pol::SegsumPlan ref;
    pol::segsum_plan({0, 3, 5}, 4, &ref);
    CHECK(plan.fold.levels.size() == 1 && ref.levels.size() == 1);
    if (plan.fold.levels.size() == 1 && ref.levels.size() == 1) {
      const auto &a = plan.fold.levels[0].chunks, &b = ref.levels[0].chunks;
      CHECK(a.size() == b.size() && a.size() == 2);
      const uint32_t row_of[2] = {1, 3};
      for (size_t k = 0; k < a.size() && k < b.size(); ++k)
        CHECK(a[k].begin == b[k].begin && a[k].len == b[k].len && a[k].dst == row_of[b[k].dst]);
    }
  }
  // ---- refusals of the plan: nothing is written ----
  {
    pol::SpmvPlan plan;
    plan.chunk = -7;
    const uint64_t bad0[] = {1, 2, 3}, dec[] = {0, 5, 4}, big[] = {0, (uint64_t)1 << 31}, ok[] = {0, 2, 3};
    CHECK(!pol::spmv_plan(bad0, 2, 4, &plan));                                          // row_ptr[0] != 0
    CHECK(!pol::spmv_plan(dec, 2, 4, &plan));                                           // decreasing
    CHECK(!pol::spmv_plan(big, 1, 4, &plan));                                           // nnz of 2^31
    CHECK(!pol::spmv_plan(ok, 0, 4, &plan) && !pol::spmv_plan(ok, 2, 0, &plan) && !pol::spmv_plan(nullptr, 2, 4, &plan));
    CHECK(!pol::spmv_plan(ok, (size_t)1 << 31, 4, &plan));                              // (refused before row_ptr is read)
    CHECK(plan.chunk == -7 && plan.chains.empty());
    CHECK(pol::spmv_plan(ok, 2, 4, &plan) && plan.chunk == 4 && plan.chains.size() == 2);
  }
  // ---- products: table + squarings per chain + multiplications per entry + fold ----
  CHECK(pol::spmv_products(65536, 65536, (size_t)1 << 20, 65536, 32, 2) == 65536.0 * 2 + 65536.0 * 32 + 1048576.0 * 16);
  CHECK(pol::spmv_products(10, 40, 94, 17, 13, 4) == 40.0 * 14 + 17.0 * 13 + 94.0 * 4 + 7.0);
  {
    // ... and equal to the per-row formula c * e_bits + m * ceil(e_bits / w) + (c - 1) summed over the rows of a real plan
    pol::SpmvPlan plan;
    CHECK(pol::spmv_plan(ragged.data(), ragged.size() - 1, 8, &plan));
    for (int e_bits : {1, 13, 32, 65})
      for (int w = 1; w <= 6; ++w) {
        double sum = 20.0 * (double)((1 << w) - 2);
        for (size_t i = 0; i + 1 < ragged.size(); ++i) {
          const size_t m = (size_t)(ragged[i + 1] - ragged[i]), c = m <= 8 ? 1 : (m + 7) / 8;
          sum += (double)(c * (size_t)e_bits + m * (size_t)((e_bits + w - 1) / w) + (c - 1));
        }
        CHECK(pol::spmv_products(ragged.size() - 1, 20, 94, plan.n_chains, e_bits, w) == sum);
      }
  }
  CHECK(pol::spmv_chains_estimate(100, 250, 4, 4) == 100 && pol::spmv_chains_estimate(100, 108, 9, 4) == 102);
  CHECK(pol::spmv_chains_estimate(65536, (size_t)1 << 20, 16, 8) == 131072);            // rows of one length: exact
  CHECK(pol::spmv_chains_estimate(1, 9, 9, 4) == 3 && pol::spmv_chains_estimate(2, 1, 1, 4) == 2);
  // ---- window: the fewest products, under the table cap; the table covers every column ----
  struct { size_t rows, cols, nnz, chains; int e_bits, G, K; } shapes[] = {
      {65536, 65536, (size_t)1 << 20, 65536, 32, 4, 18}, {1024, (size_t)1 << 20, (size_t)1 << 20, 131072, 32, 4, 18},
      {1024, 1024, 104858, 13312, 32, 4, 18}, {256, 256, 2048, 256, 32, 4, 18}, {135, 40, 600, 160, 12, 2, 19},
      {9, 20, 60, 9, 65, 8, 14}, {1, 1, 1, 1, 32, 4, 18}};
  for (const auto& s : shapes) {
    const size_t rb = (size_t)2 * s.G * s.K * 4;
    CHECK(pol::spmv_window(s.rows, s.cols, s.nnz, s.chains, s.e_bits, rb) ==
          best_window(s.rows, s.cols, s.nnz, s.chains, s.e_bits, rb));
  }
  CHECK(pol::spmv_window(65536, 65536, (size_t)1 << 20, 65536, 32, 576) == 2);          // the cap: w = 3 would be 288 MiB
  CHECK(pol::spmv_window(65536, 65536, (size_t)1 << 20, 65536, 32, 304) == 3);          // 1024-bit rows: w = 3 fits (152 MiB)
  CHECK(pol::spmv_window(1024, 1024, 104858, 13312, 32, 576) >= 4);                     // few columns, many entries: a wide window
  CHECK(pol::spmv_window(64, 300, 5000, 700, 1, 576) == 1);                             // one-bit weights: no table products at all
  CHECK(pol::spmv_window(1, (size_t)1 << 24, 100, 1, 32, 576) == 1);                    // ... and w = 1 is always allowed
  // ---- forced knobs (read at every call) ----
  setenv("PGPU_SPMV_WINDOW", "5", 1);
  setenv("PGPU_SPMV_CHUNK", "1", 1);
  CHECK(pol::spmv_window(1, 1, 1, 1, 1, 576) == 5 && pol::spmv_chunk(4, (size_t)1 << 30, 1) == 1);
  setenv("PGPU_SPMV_WINDOW", "9", 1);
  setenv("PGPU_SPMV_CHUNK", "100000", 1);
  CHECK(pol::spmv_window(1, 1, 1, 1, 1, 576) == 6 && pol::spmv_chunk(4, 1, 1) == 65536);
  setenv("PGPU_SPMV_CHUNK", "0", 1);                                                    // not a chunk: the rule
  CHECK(pol::spmv_chunk(4, 1, 1) == 4);
  unsetenv("PGPU_SPMV_WINDOW");
  unsetenv("PGPU_SPMV_CHUNK");
  CHECK(pol::spmv_chunk(4, (size_t)1 << 20, 65536) == 8);
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
