// CPU unit test of the plan of the bucket-method encrypted matvec (pailliercryptolib_amd/csrc/policy.cpp: bucket_*):
// (rows, cols, e_bits) -> window, block, product and depth bounds, the digit-aware sort.  Pure host logic -- built with
// g++ from policy.cpp alone, no device, no HIP call.  The rule is documented in DESIGN.md ("Bucket-method matvec"); the
// schedule it counts is restated in tests/test_bucket_model.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "policy.hpp"

namespace pol = pgpu::policy;
static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      ++g_failed;                                                          \
      std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);          \
    }                                                                      \
  } while (0)

// the schedule walked step by step, a product counted wherever the bound counts one: every column into its bucket, the
// two running products from the last entry down to entry 1 at both levels, the squarings, the V_k, Horner
static void brute(size_t rows, size_t cols, int e_bits, int c, int b, size_t chunk, size_t* products, size_t* depth) {
  const size_t W = (size_t)((e_bits + c - 1) / c), nb = ((size_t)1 << c) / (size_t)b;
  size_t n = 0;
  for (size_t i = 0; i < rows; ++i) {
    for (size_t t = 0; t < W; ++t) {
      n += cols;                                   // one product per column, whatever c is
      for (size_t k = 0; k < nb; ++k)
        for (size_t e = (size_t)b - 1; e >= 1; --e) n += 2;
      for (size_t k = nb - 1; k >= 1; --k) n += 2;
      for (size_t q = 1; q < (size_t)b; q <<= 1) ++n;
      for (size_t k = 0; k < nb; ++k) ++n;
    }
    for (size_t t = W - 1; t >= 1; --t) n += (size_t)c + 1;
  }
  // depth: one chain of every stage
  size_t d = 0;
  for (size_t m = cols;;) {
    d += m < chunk ? m : chunk;
    if (m <= chunk) break;
    m = (m + chunk - 1) / chunk;
  }
  for (size_t e = (size_t)b - 1; e >= 1; --e) d += 2;
  for (size_t k = nb - 1; k >= 1; --k) d += 2;
  for (size_t q = 1; q < (size_t)b; q <<= 1) ++d;
  d += nb;
  d += (W - 1) * ((size_t)c + 1);
  *products = n;
  *depth = d;
}

// the rule itself, restated: the first c of the least cost among those under the cap
static int brute_window(int G, size_t rows, size_t cols, int e_bits, size_t row_bytes) {
  int best = 1;
  double best_cost = -1;
  for (int c = 1; c <= 10; ++c) {
    const size_t W = (size_t)((e_bits + c - 1) / c);
    if (c > 1 && (double)rows * (double)W * (double)((size_t)1 << c) * (double)row_bytes > (double)pol::kMatvecTableCap) continue;
    const int b = 1 << ((c + 1) / 2);
    size_t p = 0, d = 0;
    brute(rows, cols, e_bits, c, b, (size_t)pol::segsum_chunk(G, rows * W * cols), &p, &d);
    const double cost = (double)p / (double)(1024 * 2 * (64 / G)) + pol::kBucketDepthWeight * (double)d;
    if (best_cost < 0 || cost < best_cost) {
      best_cost = cost;
      best = c;
    }
  }
  return best;
}

static uint32_t digit_of(const uint64_t* v, int e_bits, int c, size_t t) {
  uint32_t d = 0;
  for (int k = 0; k < c; ++k) {
    const size_t bit = t * (size_t)c + (size_t)k;
    if (bit < (size_t)e_bits && ((v[bit / 64] >> (bit % 64)) & 1)) d |= 1u << k;
  }
  return d;
}

int main(int argc, char** argv) {
  // "count rows cols e_bits c b": the two bounds for one plan, for tests/test_bucket_policy.py to hold against the
  // products tests/test_bucket_model.py actually issues
  if (argc == 7 && !std::strcmp(argv[1], "count")) {
    const size_t rows = std::strtoull(argv[2], nullptr, 10), cols = std::strtoull(argv[3], nullptr, 10);
    const int e_bits = std::atoi(argv[4]), c = std::atoi(argv[5]), b = std::atoi(argv[6]);
    std::printf("%.0f %zu\n", pol::bucket_products(rows, cols, e_bits, c, b), pol::bucket_depth(4, rows, cols, e_bits, c, b));
    return 0;
  }
  // ---- block, log2 ----
  const int blocks[11] = {0, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32};
  for (int c = 1; c <= 10; ++c) CHECK(pol::bucket_default_block(c) == blocks[c]);
  CHECK(pol::bucket_log2(1) == 0 && pol::bucket_log2(2) == 1 && pol::bucket_log2(3) == 1 && pol::bucket_log2(1024) == 10);
  CHECK(pol::kBucketMaxWindow == 10 && pol::kBucketDepthWeight > 0 && pol::kBucketDepthWeight <= 1.0);

  // ---- the counts against the walk, every window, the default block and b in {1, 2, 2^c} ----
  for (int c = 1; c <= 10; ++c)
    for (int b : {pol::bucket_default_block(c), 1, 2, 1 << c})
      for (int e_bits : {1, 7, 13, 32, 64, 65, 2048})
        for (size_t cols : {(size_t)1, (size_t)5, (size_t)67, (size_t)4096})
          for (size_t rows : {(size_t)1, (size_t)3}) {
            const size_t W = (size_t)((e_bits + c - 1) / c);
            size_t p = 0, d = 0;
            brute(rows, cols, e_bits, c, b, (size_t)pol::segsum_chunk(4, rows * W * cols), &p, &d);
            CHECK(pol::bucket_products(rows, cols, e_bits, c, b) == (double)p);
            CHECK(pol::bucket_depth(4, rows, cols, e_bits, c, b) == d);
          }
  // the four terms by hand: 1 x 2^20 x 32 at c = 8, b = 16 (W = 4, nb = 16)
  CHECK(pol::bucket_products(1, (size_t)1 << 20, 32, 8, 16) == 4.0 * 1048576 + 4.0 * 16 * 30 + 4.0 * (30 + 4 + 16) + 3.0 * 9);
  // depth there: chunk 32, levels of 2^20 -> 32768 -> 1024 -> 32: 4 * 32; 30; 50; 27
  CHECK(pol::segsum_chunk(4, (size_t)4 << 20) == 32);
  CHECK(pol::bucket_depth(4, 1, (size_t)1 << 20, 32, 8, 16) == 128 + 30 + 50 + 27);

  // ---- the rule at the shapes of the issue (2048-bit keys: G = 4, rows of 576 bytes) ----
  pol::BucketPlan p;
  pol::bucket_plan(4, 1, (size_t)1 << 20, 32, 576, &p);
  CHECK(p.window == 8 && p.block == 16 && p.windows == 4 && p.nb == 16);
  CHECK(p.bucket_bytes == (size_t)4 * 256 * 576);
  CHECK(p.products == pol::bucket_products(1, (size_t)1 << 20, 32, 8, 16) && p.depth == 235);
  CHECK(p.products < 33554432.0 / 7.9);          // against the 2^20 * 32 products of the table-less matvec: an eighth
  std::printf("1 x 2^20 x 32: c %d b %d products %.0f depth %zu\n", p.window, p.block, p.products, p.depth);
  for (auto shape : {std::make_pair((size_t)1, (size_t)1024), std::make_pair((size_t)1, (size_t)65536), std::make_pair((size_t)16, (size_t)65536),
                     std::make_pair((size_t)64, (size_t)1 << 20), std::make_pair((size_t)3, (size_t)67)})
    for (int e_bits : {32, 2048}) {
      pol::bucket_plan(4, shape.first, shape.second, e_bits, 576, &p);
      CHECK(p.window == brute_window(4, shape.first, shape.second, e_bits, 576));
      CHECK(p.block == pol::bucket_default_block(p.window));
      CHECK(p.windows == (size_t)((e_bits + p.window - 1) / p.window) && p.nb * (size_t)p.block == (size_t)1 << p.window);
      CHECK(p.bucket_bytes <= pol::kMatvecTableCap);
      std::printf("%zu x %zu x %d: c %d b %d W %zu products %.0f depth %zu bytes %zu\n", shape.first, shape.second, e_bits,
                  p.window, p.block, p.windows, p.products, p.depth, p.bucket_bytes);
    }
  // 1 x 1024 x 32: fewer products than the 25 087 of the matvec at its w = 3
  pol::bucket_plan(4, 1, 1024, 32, 576, &p);
  CHECK(p.products < 25087.0 * 2);
  // full-width weights on 65536 columns: far below the 65536 * 2048 of the bit-serial route
  pol::bucket_plan(4, 1, 65536, 2048, 576, &p);
  CHECK(p.products < 65536.0 * 2048 / 4);
  // (2,19) and (8,14): the geometry enters through the chains at work and the chunk only
  for (int G : {2, 8}) {
    pol::bucket_plan(G, 1, (size_t)1 << 20, 32, G == 2 ? 304 : 896, &p);
    CHECK(p.window == brute_window(G, 1, (size_t)1 << 20, 32, G == 2 ? 304 : 896));
  }

  // ---- the cap: 64 x 2^20 x 32 stays under 256 MiB, and the window the cap cuts off is not taken ----
  pol::bucket_plan(4, 64, (size_t)1 << 20, 32, 576, &p);
  CHECK(p.bucket_bytes <= pol::kMatvecTableCap && p.bucket_bytes == 64 * p.windows * ((size_t)1 << p.window) * 576);
  // 16 rows of 2048-bit weights: rows * W * 2^c * 576 passes the cap from some c on; the plan stays below it
  pol::bucket_plan(4, 16, 1024, 2048, 576, &p);
  CHECK(16.0 * 256 * 256 * 576 > (double)pol::kMatvecTableCap && p.window < 8);       // (c = 8, the choice of one row, does not fit)
  CHECK(p.bucket_bytes <= pol::kMatvecTableCap);
  CHECK(p.window == brute_window(4, 16, 1024, 2048, 576));
  // nothing fits: c = 1 all the same (the call then fails on its allocation or its 2^31 check, not in the plan)
  pol::bucket_plan(4, (size_t)1 << 20, 16, 2048, 576, &p);
  CHECK(p.window == 1 && p.block == 2 && p.nb == 1);

  // ---- W == 1 and nb == 1 ----
  pol::bucket_plan(4, 1, 100000, 1, 576, &p);
  CHECK(p.window == 1 && p.windows == 1 && p.block == 2 && p.nb == 1);
  CHECK(pol::bucket_products(1, 100, 1, 1, 2) == 100 + 2 + (0 + 1 + 1) + 0);
  CHECK(pol::bucket_products(2, 100, 8, 8, 256) == 2 * (100 + 2 * 255 + (0 + 8 + 1)));      // W == 1, nb == 1
  CHECK(pol::bucket_products(1, 100, 8, 4, 1) == 2 * (100 + 0 + (30 + 0 + 16)) + 5);         // b == 1

  // ---- ties go to the smaller window: a rule that scans rising c and replaces on a strictly lower cost only ----
  for (int e_bits : {1, 2, 3, 5, 8, 13, 32, 64, 65, 100})
    for (size_t cols : {(size_t)1, (size_t)40, (size_t)1000, (size_t)100000}) {
      pol::bucket_plan(4, 2, cols, e_bits, 576, &p);
      CHECK(p.window == brute_window(4, 2, cols, e_bits, 576));
    }

  // exact ties, constructed: with the depth weight at 0 the cost is the product count over a constant, and these shapes
  // have two windows with the same, least count (asserted here, not assumed) -- the smaller window must be taken
  {
    const struct { int e_bits; size_t cols; int lo, hi; double products; } ties[] = {
        {4, 15, 2, 4, 51}, {5, 7, 2, 3, 54}, {6, 97, 3, 6, 234}, {3, 1, 1, 3, 19}};
    for (const auto& t : ties) {
      const double plo = pol::bucket_products(1, t.cols, t.e_bits, t.lo, pol::bucket_default_block(t.lo));
      const double phi = pol::bucket_products(1, t.cols, t.e_bits, t.hi, pol::bucket_default_block(t.hi));
      CHECK(plo == t.products && phi == t.products);
      for (int c = 1; c <= 10; ++c) CHECK(pol::bucket_products(1, t.cols, t.e_bits, c, pol::bucket_default_block(c)) >= t.products);
      pol::bucket_plan(4, 1, t.cols, t.e_bits, 576, &p, 0.0);
      CHECK(p.window == t.lo && p.products == t.products);
    }
  }

  // ---- the knobs: read at every call, clamped, a forced block rounded down to a power of two, no cap ----
  setenv("PGPU_BUCKET_WINDOW", "5", 1);
  pol::bucket_plan(4, 1, (size_t)1 << 20, 32, 576, &p);
  CHECK(p.window == 5 && p.block == 8 && p.windows == 7 && p.nb == 4);
  setenv("PGPU_BUCKET_BLOCK", "7", 1);
  pol::bucket_plan(4, 1, 40, 13, 576, &p);
  CHECK(p.window == 5 && p.block == 4 && p.nb == 8);
  setenv("PGPU_BUCKET_BLOCK", "1", 1);
  pol::bucket_plan(4, 1, 40, 13, 576, &p);
  CHECK(p.block == 1 && p.nb == 32);
  setenv("PGPU_BUCKET_BLOCK", "1000", 1);
  pol::bucket_plan(4, 1, 40, 13, 576, &p);
  CHECK(p.block == 32 && p.nb == 1);
  setenv("PGPU_BUCKET_WINDOW", "99", 1);
  pol::bucket_plan(4, 1, 40, 13, 576, &p);
  CHECK(p.window == 10 && p.block == 512 && p.windows == 2);
  unsetenv("PGPU_BUCKET_BLOCK");
  pol::bucket_plan(4, (size_t)1 << 20, 16, 2048, 576, &p);      // forced: not held against the cap
  CHECK(p.window == 10 && p.block == 32 && p.bucket_bytes > pol::kMatvecTableCap);
  setenv("PGPU_BUCKET_WINDOW", "0", 1);                          // not a window: the rule
  pol::bucket_plan(4, 1, (size_t)1 << 20, 32, 576, &p);
  CHECK(p.window == 8);
  unsetenv("PGPU_BUCKET_WINDOW");
  setenv("PGPU_BUCKET_BLOCK", "2", 1);                           // a forced block alone: the window is still the rule's, for that block
  pol::bucket_plan(4, 1, 40, 13, 576, &p);
  CHECK(p.block == 2 && p.nb * 2 == (size_t)1 << p.window);
  unsetenv("PGPU_BUCKET_BLOCK");

  // ---- the sort: what segsum_sort makes of the digits as ids, never materialised ----
  uint64_t seed = 88172645463325252ull;
  auto rnd = [&] { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
  for (int c : {1, 3, 4, 8, 10})
    for (int e_bits : {1, 13, 64, 65, 128}) {
      const size_t rows = 3, cols = 37, W = (size_t)((e_bits + c - 1) / c);
      const int ww = (e_bits + 63) / 64 + 1;      // (a spare word: bits above e_bits are set and must be ignored)
      std::vector<uint64_t> w(rows * cols * (size_t)ww);
      for (auto& v : w) v = rnd();
      for (int k = 0; k < ww; ++k) w[5 * (size_t)ww + k] = 0;                  // a zero weight
      for (size_t j = 0; j < cols; ++j)
        for (int k = 0; k < ww; ++k) w[(2 * cols + j) * (size_t)ww + k] = 0;   // an all-zero row
      std::vector<uint32_t> ids(rows * W * cols);
      for (size_t i = 0; i < rows; ++i)
        for (size_t t = 0; t < W; ++t)
          for (size_t j = 0; j < cols; ++j) {
            const uint32_t d = digit_of(&w[(i * cols + j) * (size_t)ww], e_bits, c, t);
            ids[(i * W + t) * cols + j] = d ? d : pol::kSegsumNone;
          }
      std::vector<uint32_t> perm, perm2;
      std::vector<size_t> off, off2;
      CHECK(pol::segsum_sort(ids.data(), rows * W, cols, (size_t)1 << c, &perm, &off));
      pol::bucket_sort(w.data(), ww, rows, cols, e_bits, c, &perm2, &off2);
      CHECK(perm == perm2 && off == off2);
      CHECK(off2.size() == rows * W * ((size_t)1 << c) + 1);
      for (size_t g = 0; g < rows * W; ++g) CHECK(off2[g << c] == off2[(g << c) + 1]);    // bucket 0 stays empty
      CHECK(off2[(2 * W) << c] == off2.back());                                         // the all-zero row has no entry
    }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
