// CPU unit test of the plans of the signed-weight convolution and sparse product (pailliercryptolib_amd/csrc/policy.cpp:
// conv_signed_plan / spmv_signed_window / spmv_signed_products): the unsigned rules with the cap held against a table of
// 2^w + 1 rows per element and 3 (E - 1) products more for the inversion of the E elements of x.  Pure host logic -- built
// with g++ from policy.cpp alone, no device, no HIP call.  The shapes are those tools/bench_conv_signed.py measures, plus
// the edges; the rule is documented in DESIGN.md ("Signed-weight conv2d and spmv").
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

struct Shape { size_t n_img, c_in, h, w, c_out, kh, kw, sh, sw, ph, pw; };
static pol::ConvDims dims(const Shape& s) {
  const size_t d[11] = {s.n_img, s.c_in, s.h, s.w, s.c_out, s.kh, s.kw, s.sh, s.sw, s.ph, s.pw};
  pol::ConvDims g{};
  CHECK(pol::conv_geometry(d, &g));
  return g;
}

int main() {
  const size_t rb = 576;      // a pair row of a 2048-bit key: 2 * 4 * 18 limbs of 4 bytes
  // ---- conv: the bench shapes and the edges ----
  const Shape shapes[] = {
      {1024, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0}, {64, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0}, {64, 16, 14, 14, 16, 3, 3, 1, 1, 1, 1},
      {1, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0},                                           // the bench shapes
      {1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0}, {5, 2, 7, 3, 4, 3, 3, 2, 1, 1, 1}, {3, 1, 6, 6, 1, 2, 2, 2, 2, 0, 0},
      {64, 8, 30, 30, 16, 3, 3, 1, 1, 1, 1}, {9, 6, 20, 20, 16, 3, 3, 1, 1, 1, 1}};  // ... and two at the edge of the cap
  for (const Shape& s : shapes) {
    const pol::ConvDims g = dims(s);
    for (int e_bits : {1, 13, 32}) {
      pol::ConvPlan p, u;
      pol::conv_signed_plan(4, s.n_img, g.elems, g.n_o, g.taps, e_bits, rb, &p);
      pol::conv_plan(4, s.n_img, g.elems, g.n_o, g.taps, e_bits, rb, &u);
      CHECK(p.window >= 1 && p.window <= 6 && p.tile >= 1 && p.tile <= s.n_img);
      CHECK(table_bytes(p.tile * g.elems, p.window, rb) <= pol::kMatvecTableCap);
      CHECK(p.passes == (s.n_img + p.tile - 1) / p.tile && p.last == s.n_img - (p.passes - 1) * p.tile);
      // the slice rule is carried over: the unsigned call's, pass by pass
      CHECK(p.slices == pol::conv_slices(4, p.tile, g.n_o, g.taps) && p.last_slices == pol::conv_slices(4, p.last, g.n_o, g.taps));
      const double inv = 3.0 * (double)(s.n_img * g.elems - 1);
      CHECK((double)pol::invert_products(s.n_img * g.elems) == inv);
      CHECK(p.products == pol::conv_products(4, s.n_img, g.elems, g.n_o, g.taps, e_bits, p.window, p.tile) + inv);
      // no pair under the signed cap has fewer products
      bool better = false;
      for (int w = 1; w <= 6; ++w)
        for (size_t t = 1; t <= s.n_img; ++t)
          if (table_bytes(t * g.elems, w, rb) <= pol::kMatvecTableCap &&
              pol::conv_products(4, s.n_img, g.elems, g.n_o, g.taps, e_bits, w, t) + inv < p.products)
            better = true;
      CHECK(!better);
      if (p.window == u.window && p.tile == u.tile) CHECK(p.products == u.products + inv);
      else CHECK(table_bytes(u.tile * g.elems, u.window, rb) > pol::kMatvecTableCap && p.products >= u.products + inv);
    }
  }
  {
    // a shape at the edge of kMatvecTableCap: one image of 8 x 30 x 30 = 7200 elements x 64 rows x 576 B = 253 MiB fits, x 65
    // rows = 257 MiB does not -- the signed plan takes the smaller window
    const pol::ConvDims g = dims(shapes[7]);
    CHECK(g.elems == 7200 && (size_t)7200 * 64 * rb <= pol::kMatvecTableCap && table_bytes(7200, 6, rb) > pol::kMatvecTableCap);
    pol::ConvPlan p, u;
    pol::conv_plan(4, 64, g.elems, g.n_o, g.taps, 32, rb, &u);
    pol::conv_signed_plan(4, 64, g.elems, g.n_o, g.taps, 32, rb, &p);
    CHECK(u.window == 6 && u.tile == 1);
    CHECK(p.window == 5 && table_bytes(p.tile * 7200, 5, rb) <= pol::kMatvecTableCap);
    // ... and 6 x 20 x 20 = 2400 elements: three images fit the unsigned table at w = 6, two the signed -- the smaller tile
    const pol::ConvDims g2 = dims(shapes[8]);
    CHECK(g2.elems == 2400 && (size_t)3 * 2400 * 64 * rb <= pol::kMatvecTableCap && table_bytes(3 * 2400, 6, rb) > pol::kMatvecTableCap);
    pol::conv_plan(4, 9, g2.elems, g2.n_o, g2.taps, 32, rb, &u);
    pol::conv_signed_plan(4, 9, g2.elems, g2.n_o, g2.taps, 32, rb, &p);
    CHECK(u.window == 6 && u.tile == 3);
    CHECK(p.window == 6 && p.tile == 2 && p.passes == 5 && p.last == 1);
    // one oversized image: tile = 1 at the smallest window, as conv_plan leaves it
    pol::conv_signed_plan(4, 3, (size_t)1 << 20, 100, 9, 32, rb, &p);
    CHECK(p.window == 1 && p.tile == 1 && p.passes == 3);
  }
  // ---- forced knobs (read at every call): the unsigned call's own, clamped the same way ----
  setenv("PGPU_CONV_WINDOW", "2", 1);
  setenv("PGPU_CONV_TILE", "4", 1);
  setenv("PGPU_CONV_SLICES", "3", 1);
  {
    const pol::ConvDims g = dims(shapes[5]);
    pol::ConvPlan p;
    pol::conv_signed_plan(4, 5, g.elems, g.n_o, g.taps, 32, rb, &p);
    CHECK(p.window == 2 && p.tile == 4 && p.passes == 2 && p.last == 1 && p.slices == 3 && p.last_slices == 3);
    CHECK(p.products == pol::conv_products(4, 5, g.elems, g.n_o, g.taps, 32, 2, 4) + 3.0 * (double)(5 * g.elems - 1));
    setenv("PGPU_CONV_WINDOW", "9", 1);
    setenv("PGPU_CONV_TILE", "99", 1);
    setenv("PGPU_CONV_SLICES", "99", 1);
    pol::conv_signed_plan(4, 5, g.elems, g.n_o, g.taps, 32, rb, &p);
    CHECK(p.window == 6 && p.tile == 5 && p.passes == 1 && p.slices == g.taps);
  }
  unsetenv("PGPU_CONV_WINDOW");
  unsetenv("PGPU_CONV_TILE");
  unsetenv("PGPU_CONV_SLICES");

  // ---- spmv: the bench shapes and the edges ----
  struct { size_t rows, cols, nnz, chains; int e_bits; } sp[] = {
      {65536, 65536, (size_t)1 << 20, 131072, 32}, {1024, 1024, 104858, 13312, 32}, {1, 1, 1, 1, 1}, {100, 40, 300, 100, 1},
      {9, 20, 60, 33, 13}, {65536, 7200, (size_t)1 << 20, 131072, 32}};
  for (const auto& s : sp) {
    const int w = pol::spmv_signed_window(s.rows, s.cols, s.nnz, s.chains, s.e_bits, rb);
    const int u = pol::spmv_window(s.rows, s.cols, s.nnz, s.chains, s.e_bits, rb);
    CHECK(w >= 1 && w <= u);
    CHECK(w == 1 || table_bytes(s.cols, w, rb) <= pol::kMatvecTableCap);
    int best = 1;
    for (int v = 2; v <= 6 && table_bytes(s.cols, v, rb) <= pol::kMatvecTableCap; ++v)
      if (pol::spmv_products(s.rows, s.cols, s.nnz, s.chains, s.e_bits, v) < pol::spmv_products(s.rows, s.cols, s.nnz, s.chains, s.e_bits, best))
        best = v;
    CHECK(w == best);
    CHECK(w == u || table_bytes(s.cols, u, rb) > pol::kMatvecTableCap);
    // every column of x is inverted, referenced or not
    CHECK(pol::spmv_signed_products(s.rows, s.cols, s.nnz, s.chains, s.e_bits, w) ==
          pol::spmv_products(s.rows, s.cols, s.nnz, s.chains, s.e_bits, w) + 3.0 * (double)(s.cols - 1));
  }
  CHECK(pol::spmv_window(65536, 7200, (size_t)1 << 20, 131072, 32, rb) == 6);
  CHECK(pol::spmv_signed_window(65536, 7200, (size_t)1 << 20, 131072, 32, rb) == 5);     // the edge of the cap
  CHECK(pol::spmv_signed_window(65536, (size_t)1 << 20, (size_t)1 << 20, 131072, 32, rb) == 1);      // w = 1 (three rows) is always allowed
  setenv("PGPU_SPMV_WINDOW", "5", 1);
  CHECK(pol::spmv_signed_window(1, 1, 1, 1, 1, rb) == 5);
  setenv("PGPU_SPMV_WINDOW", "9", 1);
  CHECK(pol::spmv_signed_window(1, 1, 1, 1, 1, rb) == 6);
  unsetenv("PGPU_SPMV_WINDOW");
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
