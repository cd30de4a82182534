// CPU unit test of the plan of the encrypted matrix product (pailliercryptolib_amd/csrc/policy.cpp: matmul_plan /
// matmul_products / matmul_slices): (n_vec, rows, cols, e_bits) -> window, tile, slices, products.  Pure host logic -- built
// with g++ from policy.cpp alone, no device, no HIP call.  The rule is documented in policy.hpp and in DESIGN.md
// ("Encrypted matrix product"); the pass formula is restated here on its own, from the text of the rule.
#include <cstdio>
#include <cstdlib>

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

// one pass over t vectors: table + squarings + multiplications + fold, S the matvec's rule for t * rows outputs
static double pass_products(int G, size_t t, size_t rows, size_t cols, int e_bits, int w) {
  const double S = (double)pol::matvec_slices(G, t * rows, cols), nwin = (double)((e_bits + w - 1) / w);
  return (double)t * cols * (double)((1u << w) - 2) + (double)t * rows * S * e_bits + (double)t * rows * cols * nwin +
         (double)t * rows * (S - 1);
}
static double call_products(int G, size_t n_vec, size_t rows, size_t cols, int e_bits, int w, size_t tile) {
  double sum = 0;
  for (size_t v0 = 0; v0 < n_vec; v0 += tile) sum += pass_products(G, n_vec - v0 < tile ? n_vec - v0 : tile, rows, cols, e_bits, w);
  return sum;
}
// every (w, tile) under the cap, the fewest products; ties: the larger tile, then the smaller window
static void brute(int G, size_t n_vec, size_t rows, size_t cols, int e_bits, size_t rb, int* bw, size_t* bt, double* bc) {
  *bw = 0;
  for (int w = 1; w <= 6; ++w)
    for (size_t t = 1; t <= n_vec; ++t) {
      if (t * cols * ((size_t)1 << w) * rb > pol::kMatvecTableCap) break;
      const double c = call_products(G, n_vec, rows, cols, e_bits, w, t);
      if (*bw == 0 || c < *bc || (c == *bc && (t > *bt || (t == *bt && w < *bw)))) {
        *bw = w;
        *bt = t;
        *bc = c;
      }
    }
}

int main() {
  struct { int G, K; } geo[] = {{2, 19}, {4, 18}, {8, 14}};
  // ---- n_vec = 1 is the matvec: its window, its slices, tile = 1 ----
  struct { size_t rows, cols; int e_bits; } mv[] = {{1, 1024, 32}, {64, 1024, 32}, {1024, 1024, 32}, {4096, 256, 32}, {256, 512, 64},
                                                    {1, 1, 32},    {3, 1, 32},     {1, 7, 127},       {5, 33, 13},     {64, 300, 1},
                                                    {4096, 100000, 32}};
  for (const auto& g : geo)
    for (const auto& s : mv) {
      const size_t rb = (size_t)2 * g.G * g.K * 4, S = pol::matvec_slices(g.G, s.rows, s.cols);
      pol::MatmulPlan p;
      pol::matmul_plan(g.G, 1, s.rows, s.cols, s.e_bits, rb, &p);
      CHECK(p.tile == 1 && p.passes == 1 && p.last == 1);
      CHECK(p.slices == S && p.last_slices == S);
      CHECK(p.window == pol::matvec_window(s.rows, s.cols, s.e_bits, S, rb));
      CHECK(p.products == pol::matvec_products(s.rows, s.cols, s.e_bits, p.window, S));
    }
  // ---- the plan against the brute-force minimum of the documented count; the cap; tile <= n_vec; the passes ----
  struct { size_t n_vec, rows, cols; int e_bits; } shapes[] = {
      {1, 1, 1, 32},   {3, 5, 7, 32},     {7, 1, 9, 32},     {2, 17, 1, 32},    {5, 13, 33, 32},    {40, 3, 4, 32},      {5, 13, 33, 13},
      {64, 256, 256, 32}, {1024, 16, 64, 32}, {8, 8, 24, 32}, {100, 2, 3000, 32}, {37, 3, 20000, 32}, {9, 4, 100000, 32}, {300, 1, 1, 1},
      {4096, 64, 256, 32}};
  for (const auto& g : geo)
    for (const auto& s : shapes) {
      const size_t rb = (size_t)2 * g.G * g.K * 4;
      pol::MatmulPlan p;
      pol::matmul_plan(g.G, s.n_vec, s.rows, s.cols, s.e_bits, rb, &p);
      CHECK(p.window >= 1 && p.window <= 6 && p.tile >= 1 && p.tile <= s.n_vec);
      CHECK(p.tile * s.cols * ((size_t)1 << p.window) * rb <= pol::kMatvecTableCap);
      CHECK(p.passes == (s.n_vec + p.tile - 1) / p.tile && p.last == s.n_vec - (p.passes - 1) * p.tile && p.last >= 1 && p.last <= p.tile);
      CHECK(p.slices == pol::matvec_slices(g.G, p.tile * s.rows, s.cols) && p.last_slices == pol::matvec_slices(g.G, p.last * s.rows, s.cols));
      CHECK(p.slices >= 1 && p.slices <= s.cols && p.last_slices >= 1 && p.last_slices <= s.cols);
      CHECK(p.slices == pol::matmul_slices(g.G, p.tile, s.rows, s.cols));
      // the sum of the passes' formula, a short last pass included
      CHECK(p.products == call_products(g.G, s.n_vec, s.rows, s.cols, s.e_bits, p.window, p.tile));
      CHECK(p.products == pol::matmul_products(g.G, s.n_vec, s.rows, s.cols, s.e_bits, p.window, p.tile));
      int bw = 0;
      size_t bt = 0;
      double bc = 0;
      brute(g.G, s.n_vec, s.rows, s.cols, s.e_bits, rb, &bw, &bt, &bc);
      CHECK(p.window == bw && p.tile == bt && p.products == bc);
    }
  // a short last pass, by hand: 5 vectors in tiles of 2 are passes of 2, 2 and 1
  CHECK(pol::matmul_products(4, 5, 13, 33, 32, 4, 2) ==
        2 * pass_products(4, 2, 13, 33, 32, 4) + pass_products(4, 1, 13, 33, 32, 4));
  CHECK(pass_products(4, 1, 1024, 1024, 32, 4) == pol::matvec_products(1024, 1024, 32, 4, 16));
  // ---- the case the call exists for: 4096 vectors x 256 columns -> 64 rows under a 2048-bit key ----
  {
    const size_t n_vec = 4096, rows = 64, cols = 256, rb = 576;
    pol::MatmulPlan p;
    pol::matmul_plan(4, n_vec, rows, cols, 32, rb, &p);
    CHECK(p.window > 1 && p.tile < n_vec && p.passes > 1);
    CHECK(p.tile * cols * ((size_t)1 << p.window) * rb <= pol::kMatvecTableCap);
    CHECK((p.tile + 1) * cols * ((size_t)1 << p.window) * rb > pol::kMatvecTableCap || p.tile == n_vec ||
          pol::matmul_products(4, n_vec, rows, cols, 32, p.window, p.tile + 1) > p.products);
    // the spmv formulation of the same flat matrix: n_vec * rows CSR rows of cols entries over n_vec * cols columns -- the
    // table over all columns holds the window at 1
    const size_t srows = n_vec * rows, scols = n_vec * cols, nnz = srows * cols;
    const int chunk = pol::spmv_chunk(4, nnz, srows);
    const size_t chains = pol::spmv_chains_estimate(srows, nnz, cols, chunk);
    const int sw = pol::spmv_window(srows, scols, nnz, chains, 32, rb);
    CHECK(sw == 1);
    CHECK(pol::spmv_products(srows, scols, nnz, chains, 32, sw) > 2 * p.products);
    std::printf("4096 x 256 -> 64: window %d tile %zu passes %zu slices %zu products %.0f (spmv: window %d, %.0f)\n", p.window, p.tile,
                p.passes, p.slices, p.products, sw, pol::spmv_products(srows, scols, nnz, chains, 32, sw));
  }
  // ---- one vector whose table at w = 1 exceeds the cap: tile = 1, w = 1 ----
  {
    pol::MatmulPlan p;
    pol::matmul_plan(4, 3, 2, (size_t)1 << 20, 32, 576, &p);      // 2^20 columns x 2 entries x 576 B = 1.1 GiB
    CHECK(p.tile == 1 && p.window == 1 && p.passes == 3 && p.last == 1);
    pol::matmul_plan(4, 3, 2, (size_t)1 << 17, 32, 576, &p);      // 2^17 columns: w = 1 fits once, w = 2 does not
    CHECK(p.window == 1 && p.tile == 1);
    CHECK(p.tile * ((size_t)1 << 17) * 2 * 576 <= pol::kMatvecTableCap);
  }
  // ---- forced knobs (read at every call), clamped to their legal ranges ----
  {
    pol::MatmulPlan p;
    setenv("PGPU_MATMUL_WINDOW", "4", 1);
    setenv("PGPU_MATMUL_TILE", "2", 1);
    setenv("PGPU_MATMUL_SLICES", "5", 1);
    pol::matmul_plan(4, 5, 13, 33, 32, 576, &p);
    CHECK(p.window == 4 && p.tile == 2 && p.passes == 3 && p.last == 1 && p.slices == 5 && p.last_slices == 5);
    CHECK(pol::matmul_slices(4, 2, 13, 33) == 5 && pol::matmul_slices(4, 2, 13, 3) == 3);
    const double nwin = 8, pass2 = 2 * 33 * 14.0 + 2 * 13 * 5 * 32.0 + 2 * 13 * 33 * nwin + 2 * 13 * 4.0,
                 pass1 = 33 * 14.0 + 13 * 5 * 32.0 + 13 * 33 * nwin + 13 * 4.0;
    CHECK(p.products == 2 * pass2 + pass1);
    setenv("PGPU_MATMUL_WINDOW", "9", 1);
    setenv("PGPU_MATMUL_TILE", "77", 1);
    setenv("PGPU_MATMUL_SLICES", "1000", 1);
    pol::matmul_plan(4, 5, 13, 33, 32, 576, &p);
    CHECK(p.window == 6 && p.tile == 5 && p.passes == 1 && p.slices == 33);
    unsetenv("PGPU_MATMUL_WINDOW");
    pol::matmul_plan(4, 5, 13, 33, 32, 576, &p);      // tile and slices forced, the window free: the best of the six
    CHECK(p.tile == 5 && p.slices == 33);
    for (int w = 1; w <= 6; ++w) CHECK(p.products <= pol::matmul_products(4, 5, 13, 33, 32, w, 5));
    unsetenv("PGPU_MATMUL_TILE");
    unsetenv("PGPU_MATMUL_SLICES");
    // the matvec's knobs are the matvec's: they do not move this plan
    pol::MatmulPlan q, r;
    pol::matmul_plan(4, 5, 13, 33, 32, 576, &q);
    setenv("PGPU_MATVEC_WINDOW", "1", 1);
    setenv("PGPU_MATVEC_SLICES", "1", 1);
    pol::matmul_plan(4, 5, 13, 33, 32, 576, &r);
    unsetenv("PGPU_MATVEC_WINDOW");
    unsetenv("PGPU_MATVEC_SLICES");
    CHECK(q.window == r.window && q.tile == r.tile && q.slices == r.slices && q.products == r.products);
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
