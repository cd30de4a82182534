// CPU unit test of the plans of the signed-weight matvec and matmul (pailliercryptolib_amd/csrc/policy.cpp:
// matvec_signed_window / matvec_signed_products / matmul_signed_plan): the unsigned slices and tile rules, the window that
// minimises the same product count under the same cap for a table of 2^w + 1 rows per element, and 3 (E - 1) products more
// for the inversion of E elements.  Pure host logic -- built with g++ from policy.cpp alone, no device, no HIP call.  The
// shapes are those tools/bench_matvec_signed.py measures, plus the edges; the rule is documented in DESIGN.md
// ("Signed-weight matvec and matmul").
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

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

static size_t table_bytes(size_t elems, int w, size_t rb) { return elems * (((size_t)1 << w) + 1) * rb; }

static int best_window(size_t rows, size_t cols, int e_bits, size_t S, size_t rb) {
  int best = 1;
  for (int w = 2; w <= 6; ++w)
    if (table_bytes(cols, w, rb) <= pol::kMatvecTableCap &&
        pol::matvec_signed_products(rows, cols, e_bits, w, S) < pol::matvec_signed_products(rows, cols, e_bits, best, S))
      best = w;
  return best;
}

int main() {
  const size_t rb = 576;      // a pair row of a 2048-bit key: 2 * 4 * 18 limbs of 4 bytes
  // ---- matvec: the bench shapes and the edges ----
  struct { size_t rows, cols; int e_bits, G, K; } shapes[] = {
      {1024, 1024, 32, 4, 18}, {4096, 256, 32, 4, 18}, {1, 1024, 32, 4, 18},          // the bench shapes
      {1, 7, 32, 4, 18}, {3, 1, 32, 4, 18}, {1, 1, 1, 4, 18}, {64, 300, 1, 4, 18},    // one row, one column, e_bits = 1
      {5, 33, 70, 4, 18}, {256, 512, 32, 8, 14}, {1024, 1024, 32, 2, 19}};
  for (const auto& s : shapes) {
    const size_t r = (size_t)2 * s.G * s.K * 4, S = pol::matvec_slices(s.G, s.rows, s.cols);
    const int w = pol::matvec_signed_window(s.rows, s.cols, s.e_bits, S, r);
    CHECK(w == best_window(s.rows, s.cols, s.e_bits, S, r));
    CHECK(w == 1 || table_bytes(s.cols, w, r) <= pol::kMatvecTableCap);
    // the count: the unsigned schedule's plus the inversion
    CHECK(pol::matvec_signed_products(s.rows, s.cols, s.e_bits, w, S) ==
          pol::matvec_products(s.rows, s.cols, s.e_bits, w, S) + 3.0 * (double)(s.cols - 1));
    CHECK(pol::invert_products(s.cols) == 3 * (s.cols - 1));
  }
  CHECK(pol::matvec_signed_window(1024, 1024, 32, 16, rb) == 6 && table_bytes(1024, 6, rb) == (size_t)1024 * 65 * 576);
  CHECK(pol::matvec_signed_window(1, 1024, 32, 256, rb) == pol::matvec_window(1, 1024, 32, 256, rb));
  CHECK(pol::matvec_signed_window(64, 300, 1, 1, rb) == 1);        // e_bits = 1: digits -1 / 0, rows one, x, x^-1, no table product
  CHECK(pol::matvec_signed_products(7, 300, 1, 1, 1) == 7.0 * 1 + 7.0 * 300 + 3.0 * 299);
  CHECK(pol::matvec_signed_products(1, 1, 32, 3, 1) == 6.0 + 32 + 11 + 0);       // one element: nothing to invert in a batch
  CHECK(pol::matvec_signed_products(1024, 1024, 32, 4, 16) ==
        1024.0 * 14 + 1024.0 * 16 * 32 + 1024.0 * 1024 * 8 + 1024.0 * 15 + 3.0 * 1023);
  // a table that fits the cap only at a smaller window than the unsigned call's: 7200 columns x 64 rows x 576 B = 253 MiB
  // fits, x 65 rows = 257 MiB does not
  CHECK((size_t)7200 * 64 * rb <= pol::kMatvecTableCap && table_bytes(7200, 6, rb) > pol::kMatvecTableCap);
  CHECK(pol::matvec_window(4096, 7200, 32, 1, rb) == 6);
  CHECK(pol::matvec_signed_window(4096, 7200, 32, 1, rb) == 5);
  CHECK(pol::matvec_signed_window(4096, (size_t)1 << 20, 32, 1, rb) == 1);      // w = 1 (three rows) is always allowed
  // ---- forced knobs (read at every call): the unsigned calls' own ----
  setenv("PGPU_MATVEC_WINDOW", "5", 1);
  CHECK(pol::matvec_signed_window(1, 1, 1, 1, rb) == 5);
  setenv("PGPU_MATVEC_WINDOW", "9", 1);
  CHECK(pol::matvec_signed_window(1, 1, 1, 1, rb) == 6);
  unsetenv("PGPU_MATVEC_WINDOW");
  CHECK(pol::matvec_signed_window(1024, 1024, 32, 16, rb) == 6);

  // ---- matmul: the bench shapes and the edges ----
  struct { size_t n_vec, rows, cols; int e_bits; } mm[] = {
      {1024, 16, 64, 32}, {64, 256, 256, 32}, {9, 5, 7, 32}, {3, 1, 1, 1}, {1, 17, 9, 32}, {40, 8, 3000, 32}};
  for (const auto& s : mm) {
    pol::MatmulPlan p, u;
    pol::matmul_signed_plan(4, s.n_vec, s.rows, s.cols, s.e_bits, rb, &p);
    pol::matmul_plan(4, s.n_vec, s.rows, s.cols, s.e_bits, rb, &u);
    CHECK(p.window >= 1 && p.window <= 6 && p.tile >= 1 && p.tile <= s.n_vec);
    CHECK(table_bytes(p.tile * s.cols, p.window, rb) <= pol::kMatvecTableCap);
    CHECK(p.passes == (s.n_vec + p.tile - 1) / p.tile && p.last == s.n_vec - (p.passes - 1) * p.tile);
    CHECK(p.slices == pol::matmul_slices(4, p.tile, s.rows, s.cols) && p.last_slices == pol::matmul_slices(4, p.last, s.rows, s.cols));
    const double inv = 3.0 * (double)(s.n_vec * s.cols - 1);
    CHECK(p.products == pol::matmul_products(4, s.n_vec, s.rows, s.cols, s.e_bits, p.window, p.tile) + inv);
    // no pair under the signed cap has fewer products
    bool better = false;
    for (int w = 1; w <= 6; ++w)
      for (size_t t = 1; t <= s.n_vec; ++t)
        if (table_bytes(t * s.cols, w, rb) <= pol::kMatvecTableCap &&
            pol::matmul_products(4, s.n_vec, s.rows, s.cols, s.e_bits, w, t) + inv < p.products)
          better = true;
    CHECK(!better);
    if (p.window == u.window && p.tile == u.tile) CHECK(p.products == u.products + inv);
    else CHECK(table_bytes(u.tile * s.cols, u.window, rb) > pol::kMatvecTableCap && p.products >= u.products + inv);
  }
  {
    // one vector: the signed matvec's window and slices
    pol::MatmulPlan p;
    pol::matmul_signed_plan(4, 1, 17, 9, 32, rb, &p);
    const size_t S = pol::matvec_slices(4, 17, 9);
    CHECK(p.tile == 1 && p.slices == S && p.window == pol::matvec_signed_window(17, 9, 32, S, rb));
    CHECK(p.products == pol::matvec_signed_products(17, 9, 32, p.window, S));
    // the longer table moves the plan: 40 vectors of 3000 columns at w = 6 are 40 * 3000 * 64 * 576 B > the cap either way,
    // so the tile is what the cap allows -- one vector fewer per row of the table than the unsigned plan may hold
    pol::MatmulPlan q, u;
    pol::matmul_signed_plan(4, 40, 8, 3000, 32, rb, &q);
    pol::matmul_plan(4, 40, 8, 3000, 32, rb, &u);
    CHECK(q.tile * 3000 * (((size_t)1 << q.window) + 1) * rb <= pol::kMatvecTableCap);
    CHECK(q.window < u.window || q.tile <= u.tile);
  }
  setenv("PGPU_MATMUL_WINDOW", "2", 1);
  setenv("PGPU_MATMUL_TILE", "4", 1);
  setenv("PGPU_MATMUL_SLICES", "3", 1);
  {
    pol::MatmulPlan p;
    pol::matmul_signed_plan(4, 9, 5, 7, 32, rb, &p);
    CHECK(p.window == 2 && p.tile == 4 && p.passes == 3 && p.last == 1 && p.slices == 3 && p.last_slices == 3);
    CHECK(p.products == pol::matmul_products(4, 9, 5, 7, 32, 2, 4) + 3.0 * 62);
  }
  unsetenv("PGPU_MATMUL_WINDOW");
  unsetenv("PGPU_MATMUL_TILE");
  unsetenv("PGPU_MATMUL_SLICES");
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
