// CPU unit test of the plan of the encrypted 2-D convolution (pailliercryptolib_amd/csrc/policy.cpp: conv_plan /
// conv_products / conv_slices / conv_geometry): shape and e_bits -> window, tile, slices, products.  Pure host logic -- built
// with g++ from policy.cpp alone, no device, no HIP call.  The rule is documented in policy.hpp and in DESIGN.md
// ("Encrypted 2-D convolution"); the pass formula is restated here on its own, from the text of the rule.
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

struct Shape {
  size_t n_img, c_in, h, w, c_out, kh, kw, sh, sw, ph, pw;
  int e_bits;
};
struct Sizes {
  size_t oh, ow, elems, n_o, taps;
};
static Sizes sizes(const Shape& s) {
  Sizes z;
  z.oh = (s.h + 2 * s.ph - s.kh) / s.sh + 1;
  z.ow = (s.w + 2 * s.pw - s.kw) / s.sw + 1;
  z.elems = s.c_in * s.h * s.w;
  z.n_o = s.c_out * z.oh * z.ow;
  z.taps = s.c_in * s.kh * s.kw;
  return z;
}
// one pass over t images: table + squarings + multiplications + fold, S the matvec's rule for t * n_o outputs over taps
static double pass_products(int G, size_t t, const Sizes& z, int e_bits, int w) {
  const double S = (double)pol::matvec_slices(G, t * z.n_o, z.taps), nwin = (double)((e_bits + w - 1) / w);
  return (double)t * z.elems * (double)((1u << w) - 2) + (double)t * z.n_o * S * e_bits + (double)t * z.n_o * z.taps * nwin +
         (double)t * z.n_o * (S - 1);
}
static double call_products(int G, size_t n_img, const Sizes& z, int e_bits, int w, size_t tile) {
  double sum = 0;
  for (size_t i0 = 0; i0 < n_img; i0 += tile) sum += pass_products(G, n_img - i0 < tile ? n_img - i0 : tile, z, e_bits, w);
  return sum;
}
// every (w, tile) under the cap, the fewest products; ties: the larger tile, then the smaller window
static void brute(int G, size_t n_img, const Sizes& z, int e_bits, size_t rb, int* bw, size_t* bt, double* bc) {
  *bw = 0;
  for (int w = 1; w <= 6; ++w)
    for (size_t t = 1; t <= n_img; ++t) {
      if (t * z.elems * ((size_t)1 << w) * rb > pol::kMatvecTableCap) break;
      const double c = call_products(G, n_img, z, e_bits, w, t);
      if (*bw == 0 || c < *bc || (c == *bc && (t > *bt || (t == *bt && w < *bw)))) {
        *bw = w;
        *bt = t;
        *bc = c;
      }
    }
}
static bool geometry(const Shape& s, pol::ConvDims* g) {
  const size_t d[11] = {s.n_img, s.c_in, s.h, s.w, s.c_out, s.kh, s.kw, s.sh, s.sw, s.ph, s.pw};
  return pol::conv_geometry(d, g);
}

int main() {
  struct { int G, K; } geo[] = {{2, 19}, {4, 18}, {8, 14}};
  // ---- the sizes of a shape, and what a shape alone is refused for ----
  {
    pol::ConvDims g;
    CHECK(geometry({5, 2, 7, 3, 4, 3, 3, 2, 1, 1, 1, 13}, &g));
    CHECK(g.oh == 4 && g.ow == 3 && g.elems == 42 && g.taps == 18 && g.n_o == 48 && g.x_count == 210 && g.w_count == 72 && g.out_count == 240);
    CHECK(geometry({1, 1, 8, 7, 1, 3, 3, 2, 2, 0, 0, 13}, &g) && g.oh == 3 && g.ow == 3);      // the floor leaves a row and a column unread
    CHECK(geometry({1, 1, 3, 3, 1, 3, 3, 1, 1, 2, 2, 13}, &g) && g.oh == 5 && g.ow == 5);      // maximal legal padding
    CHECK(geometry({1, 1, 1, 9, 1, 1, 3, 1, 1, 0, 1, 13}, &g) && g.oh == 1 && g.ow == 9);      // conv1d
    CHECK(geometry({1, 1, 4, 4, 1, 2, 2, 1000, 7, 0, 0, 13}, &g) && g.oh == 1 && g.ow == 1);   // a stride beyond the image
    const Shape ok{2, 3, 5, 4, 2, 3, 2, 1, 1, 1, 0, 13};
    CHECK(geometry(ok, &g));
    for (int f = 0; f < 9; ++f) {      // any dimension or stride equal to 0
      size_t d[11] = {ok.n_img, ok.c_in, ok.h, ok.w, ok.c_out, ok.kh, ok.kw, ok.sh, ok.sw, ok.ph, ok.pw};
      d[f] = 0;
      CHECK(!pol::conv_geometry(d, &g));
    }
    CHECK(!geometry({1, 1, 5, 5, 1, 3, 3, 1, 1, 3, 0, 13}, &g));      // pad_h >= kh
    CHECK(!geometry({1, 1, 5, 5, 1, 3, 3, 1, 1, 0, 3, 13}, &g));      // pad_w >= kw
    CHECK(!geometry({1, 1, 2, 5, 1, 5, 3, 1, 1, 1, 0, 13}, &g));      // kh > h + 2 pad_h
    CHECK(!geometry({1, 1, 5, 2, 1, 3, 5, 1, 1, 0, 1, 13}, &g));      // kw > w + 2 pad_w
    const size_t big = (size_t)1 << 40;
    CHECK(!geometry({big, big, 4, 4, 1, 2, 2, 1, 1, 0, 0, 13}, &g));  // n_img * c_in * h * w beyond size_t
    CHECK(!geometry({big, 1, 4, 4, big, 2, 2, 1, 1, 0, 0, 13}, &g));  // n_img * c_out * oh * ow beyond size_t
    CHECK(!geometry({1, 1, big, 4, 1, 2, 2, 1, 1, 0, 0, 13}, &g));    // an image side of 2^30 or more
  }
  // ---- a kernel equal to the image, no padding, n_img = 1 is the matvec: rows = c_out, cols = c_in*h*w ----
  const Shape mv[] = {{1, 2, 4, 5, 3, 4, 5, 1, 1, 0, 0, 32}, {1, 1, 32, 32, 64, 32, 32, 1, 1, 0, 0, 32}, {1, 3, 7, 9, 1024, 7, 9, 3, 2, 0, 0, 13},
                      {1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 32}, {1, 1, 1, 7, 1, 1, 7, 1, 1, 0, 0, 127}, {1, 16, 80, 80, 4096, 80, 80, 1, 1, 0, 0, 32}};
  for (const auto& g : geo)
    for (const auto& s : mv) {
      const Sizes z = sizes(s);
      const size_t rb = (size_t)2 * g.G * g.K * 4, rows = s.c_out, cols = z.elems, S = pol::matvec_slices(g.G, rows, cols);
      CHECK(z.oh == 1 && z.ow == 1 && z.taps == z.elems && z.n_o == rows);
      pol::ConvPlan p;
      pol::conv_plan(g.G, 1, z.elems, z.n_o, z.taps, s.e_bits, rb, &p);
      CHECK(p.tile == 1 && p.passes == 1 && p.last == 1);
      CHECK(p.slices == S && p.last_slices == S);
      CHECK(p.window == pol::matvec_window(rows, cols, s.e_bits, S, rb));
      CHECK(p.products == pol::matvec_products(rows, cols, s.e_bits, p.window, S));
    }
  // ---- the plan against the brute-force minimum of the documented count; the cap; tile <= n_img; the passes ----
  const Shape shapes[] = {{1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 32},   {1, 1, 1, 9, 1, 1, 3, 1, 1, 0, 1, 32},  {2, 3, 5, 4, 2, 3, 2, 1, 1, 1, 0, 32},
                          {3, 1, 6, 6, 1, 2, 2, 2, 2, 0, 0, 1},    {1, 1, 8, 7, 1, 3, 3, 2, 2, 0, 0, 32},  {1, 2, 4, 5, 3, 4, 5, 1, 1, 0, 0, 32},
                          {1, 3, 4, 5, 2, 1, 1, 1, 1, 0, 0, 32},   {1, 1, 3, 3, 1, 3, 3, 1, 1, 2, 2, 32},  {5, 2, 7, 3, 4, 3, 3, 2, 1, 1, 1, 13},
                          {64, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0, 32}, {1024, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0, 32},
                          {64, 16, 14, 14, 16, 3, 3, 1, 1, 1, 1, 32}, {300, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1}, {37, 3, 90, 80, 2, 3, 3, 1, 1, 1, 1, 32},
                          {9, 4, 160, 160, 4, 3, 3, 2, 2, 1, 1, 32}, {7, 1, 1, 4000, 1, 1, 9, 1, 4, 0, 4, 64}};
  for (const auto& g : geo)
    for (const auto& s : shapes) {
      const Sizes z = sizes(s);
      const size_t rb = (size_t)2 * g.G * g.K * 4;
      pol::ConvDims d;
      CHECK(geometry(s, &d) && d.oh == z.oh && d.ow == z.ow && d.elems == z.elems && d.n_o == z.n_o && d.taps == z.taps);
      pol::ConvPlan p;
      pol::conv_plan(g.G, s.n_img, z.elems, z.n_o, z.taps, s.e_bits, rb, &p);
      CHECK(p.window >= 1 && p.window <= 6 && p.tile >= 1 && p.tile <= s.n_img);
      CHECK(p.tile * z.elems * ((size_t)1 << p.window) * rb <= pol::kMatvecTableCap);
      CHECK(p.passes == (s.n_img + p.tile - 1) / p.tile && p.last == s.n_img - (p.passes - 1) * p.tile && p.last >= 1 && p.last <= p.tile);
      CHECK(p.slices == pol::matvec_slices(g.G, p.tile * z.n_o, z.taps) && p.last_slices == pol::matvec_slices(g.G, p.last * z.n_o, z.taps));
      CHECK(p.slices >= 1 && p.slices <= z.taps && p.last_slices >= 1 && p.last_slices <= z.taps);
      CHECK(p.slices == pol::conv_slices(g.G, p.tile, z.n_o, z.taps));
      // the sum of the passes' formula, a short last pass included
      CHECK(p.products == call_products(g.G, s.n_img, z, s.e_bits, p.window, p.tile));
      CHECK(p.products == pol::conv_products(g.G, s.n_img, z.elems, z.n_o, z.taps, s.e_bits, p.window, p.tile));
      int bw = 0;
      size_t bt = 0;
      double bc = 0;
      brute(g.G, s.n_img, z, s.e_bits, rb, &bw, &bt, &bc);
      CHECK(p.window == bw && p.tile == bt && p.products == bc);
    }
  // a short last pass has its own S, by hand: 5 images in tiles of 2 are passes of 2, 2 and 1; and 3 images of 16x16 with
  // 16 filters of 5x5 (2304 outputs an image) in tiles of 2 under (4,18), where the pass of 2 images and the last pass of 1
  // image fill the chip with different slice counts
  {
    const Sizes z = sizes({5, 2, 7, 3, 4, 3, 3, 2, 1, 1, 1, 13});
    CHECK(pol::conv_products(8, 5, z.elems, z.n_o, z.taps, 13, 4, 2) == 2 * pass_products(8, 2, z, 13, 4) + pass_products(8, 1, z, 13, 4));
    const Sizes y = sizes({3, 1, 16, 16, 16, 5, 5, 1, 1, 0, 0, 32});
    CHECK(pol::matvec_slices(4, 2 * y.n_o, y.taps) != pol::matvec_slices(4, 1 * y.n_o, y.taps));
    setenv("PGPU_CONV_TILE", "2", 1);
    pol::ConvPlan p;
    pol::conv_plan(4, 3, y.elems, y.n_o, y.taps, 32, 576, &p);
    unsetenv("PGPU_CONV_TILE");
    CHECK(p.tile == 2 && p.passes == 2 && p.last == 1);
    CHECK(p.slices == pol::matvec_slices(4, 2 * y.n_o, y.taps) && p.last_slices == pol::matvec_slices(4, y.n_o, y.taps) && p.slices != p.last_slices);
    CHECK(p.products == pass_products(4, 2, y, 32, p.window) + pass_products(4, 1, y, 32, p.window));
  }
  // ---- the case the call exists for: a minibatch of 1x28x28 images, 8 filters of 5x5, 2048-bit key, 32-bit weights ----
  for (size_t n_img : {(size_t)1, (size_t)64, (size_t)1024}) {
    const Shape s{n_img, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0, 32};
    const Sizes z = sizes(s);
    const size_t rb = 576;
    pol::ConvPlan p;
    pol::conv_plan(4, n_img, z.elems, z.n_o, z.taps, 32, rb, &p);
    CHECK(p.window > 1);
    CHECK(p.tile * z.elems * ((size_t)1 << p.window) * rb <= pol::kMatvecTableCap);
    // the spmv formulation of the same map: n_img * n_o CSR rows of taps entries over n_img * elems columns, asked of the
    // spmv's own plan functions
    const size_t srows = n_img * z.n_o, scols = n_img * z.elems, nnz = srows * z.taps;
    const int chunk = pol::spmv_chunk(4, nnz, srows);
    const size_t chains = pol::spmv_chains_estimate(srows, nnz, z.taps, chunk);
    const int sw = pol::spmv_window(srows, scols, nnz, chains, 32, rb);
    const double sp = pol::spmv_products(srows, scols, nnz, chains, 32, sw);
    std::printf("%zu x 1x28x28 * 8 x 5x5: window %d tile %zu passes %zu slices %zu products %.0f (spmv: window %d, %.0f, ratio %.2f)\n",
                n_img, p.window, p.tile, p.passes, p.slices, p.products, sw, sp, sp / p.products);
    if (n_img == 1024) {
      CHECK(sw == 1);           // the table over all of x holds the spmv at window 1 ...
      CHECK(p.window >= 4);     // ... where a tile of images affords a wide one
      CHECK(p.tile < n_img && p.passes > 1);
      CHECK(sp > 2 * p.products);
    }
    if (n_img == 64) CHECK(sw < p.window);
  }
  // ---- one image whose table at w = 1 exceeds the cap: tile = 1, w = 1 ----
  {
    pol::ConvPlan p;
    pol::conv_plan(4, 3, (size_t)1 << 20, 2, 9, 32, 576, &p);      // 2^20 elements x 2 entries x 576 B = 1.1 GiB
    CHECK(p.tile == 1 && p.window == 1 && p.passes == 3 && p.last == 1);
    pol::conv_plan(4, 3, (size_t)1 << 17, 2, 9, 32, 576, &p);      // 2^17 elements: w = 1 fits once, w = 2 does not
    CHECK(p.window == 1 && p.tile == 1);
    CHECK(p.tile * ((size_t)1 << 17) * 2 * 576 <= pol::kMatvecTableCap);
  }
  // ---- forced knobs (read at every call), clamped to their legal ranges ----
  {
    const Sizes z = sizes({5, 2, 7, 3, 4, 3, 3, 2, 1, 1, 1, 13});      // elems 42, n_o 48, taps 18
    pol::ConvPlan p;
    setenv("PGPU_CONV_WINDOW", "4", 1);
    setenv("PGPU_CONV_TILE", "2", 1);
    setenv("PGPU_CONV_SLICES", "5", 1);
    pol::conv_plan(4, 5, z.elems, z.n_o, z.taps, 13, 576, &p);
    CHECK(p.window == 4 && p.tile == 2 && p.passes == 3 && p.last == 1 && p.slices == 5 && p.last_slices == 5);
    CHECK(pol::conv_slices(4, 2, 48, 18) == 5 && pol::conv_slices(4, 2, 48, 3) == 3);
    const double nwin = 4, pass2 = 2 * 42 * 14.0 + 2 * 48 * 5 * 13.0 + 2 * 48 * 18 * nwin + 2 * 48 * 4.0,
                 pass1 = 42 * 14.0 + 48 * 5 * 13.0 + 48 * 18 * nwin + 48 * 4.0;
    CHECK(p.products == 2 * pass2 + pass1);
    setenv("PGPU_CONV_WINDOW", "9", 1);
    setenv("PGPU_CONV_TILE", "77", 1);
    setenv("PGPU_CONV_SLICES", "1000", 1);
    pol::conv_plan(4, 5, z.elems, z.n_o, z.taps, 13, 576, &p);
    CHECK(p.window == 6 && p.tile == 5 && p.passes == 1 && p.slices == 18);
    unsetenv("PGPU_CONV_WINDOW");
    pol::conv_plan(4, 5, z.elems, z.n_o, z.taps, 13, 576, &p);      // tile and slices forced, the window free: the best of the six
    CHECK(p.tile == 5 && p.slices == 18);
    for (int w = 1; w <= 6; ++w) CHECK(p.products <= pol::conv_products(4, 5, z.elems, z.n_o, z.taps, 13, w, 5));
    unsetenv("PGPU_CONV_TILE");
    unsetenv("PGPU_CONV_SLICES");
    // the matmul's and the matvec's knobs are theirs: they do not move this plan
    pol::ConvPlan q, r;
    pol::conv_plan(4, 5, z.elems, z.n_o, z.taps, 13, 576, &q);
    setenv("PGPU_MATMUL_WINDOW", "1", 1);
    setenv("PGPU_MATMUL_TILE", "1", 1);
    setenv("PGPU_MATMUL_SLICES", "1", 1);
    setenv("PGPU_MATVEC_WINDOW", "1", 1);
    setenv("PGPU_MATVEC_SLICES", "1", 1);
    pol::conv_plan(4, 5, z.elems, z.n_o, z.taps, 13, 576, &r);
    unsetenv("PGPU_MATMUL_WINDOW");
    unsetenv("PGPU_MATMUL_TILE");
    unsetenv("PGPU_MATMUL_SLICES");
    unsetenv("PGPU_MATVEC_WINDOW");
    unsetenv("PGPU_MATVEC_SLICES");
    CHECK(q.window == r.window && q.tile == r.tile && q.slices == r.slices && q.products == r.products);
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
