// pailliercryptolib_amd -- the signed-weight encrypted 2-D convolution on resident ciphertexts (pgpu_batch_ct_conv2d_signed):
//     out[n][co][oy][ox] = prod_{ci,ky,kx} x[n][ci][oy*sh + ky - ph][ox*sw + kx - pw]^w[co][ci][ky][kx]  mod n^2,
// w[co][ci][ky][kx] a SIGNED integer, two's complement in e_bits bits (a tap outside the image contributes one, whatever
// its weight's sign).  conv_kernel of hensel_conv.hpp on the tables and digits of hensel_signed.hpp:
//   * the tables T[e][.] over [x_e ; x_e^-1] of a TILE of whole images -- 2^w + 1 rows per element: row 0 = one, rows 1..h
//     = x^1..x^h, rows h+1..2h = x^-1..x^-h, h = 2^(w-1) -- are built by the unchanged matvec_signed_table_kernel over the
//     tile's contiguous range of x and of x^-1 (the host inverts ALL of x once, before the first pass);
//   * the schedule is conv_kernel's, unchanged: flat output numbering across the groups of a wavefront, wavefront-uniform
//     tap slices walked with (ci, ky, kx) in uniform registers, from the top window down w squarings and one product per
//     tap, the two-ahead digit fetch and the one-ahead entry load, dead groups clamped and not stored;
//   * the row of a tap is signed_digit_row of its weight's Booth digit (row d, or row h - d for d < 0), and the table
//     stride counts elements of 2^w + 1 rows;
//   * a tap outside the image takes row 0 on a clamped, valid element, whatever its weight: T[.][0] is the row of one.  No
//     branch on `inside`, and none on a digit, around a product that exchanges data across the group.
// The schedule is restated in plain integers in tests/test_conv_signed_model.py.
//
// The arithmetic is seq_pairmul of hensel_seq.hpp on pair rows.  The table is indexed by digits of the caller's PLAINTEXT
// filters and by positions derived from the shape (the indexed access of the default table_gather_policy; the host refuses
// the call under the masked policy).
#ifndef PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_CONV_SIGNED_HPP_
#define PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_CONV_SIGNED_HPP_

#include "hensel_conv.hpp"      // ConvPos
#include "hensel_signed.hpp"    // signed_digit_row

namespace pgpu {

// One wavefront = 64/G consecutive outputs of ONE tap slice, as in conv_kernel.
template <int G, int K>
__global__ __launch_bounds__(kWGThreads, 2) void conv_signed_kernel(ConvArgs A) {
  constexpr int IPW = kWave / G, L2 = G * K, LQ = 2 * L2;
  raise_wave_priority();
  __shared__ __attribute__((aligned(16))) uint32_t qs_[kWavesPerWG][IPW][G * kAbPad];
  __shared__ __attribute__((aligned(16))) uint32_t ts_[kWavesPerWG][kWave][kAbPad];
  const int lane = threadIdx.x % kWave, wv = threadIdx.x / kWave;
  const int grp = lane / G, x = lane % G;
  uint32_t* qs = qs_[wv][grp];
  uint32_t* ts = ts_[wv][lane];
  uint32_t sel0 = x == 0 ? 1u : 0u;
  asm("" : "+v"(sel0));
  const size_t wave_id = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerWG + wv));
  const size_t out_blocks = (A.n_out + IPW - 1) / IPW;
  const size_t slice = wave_id / out_blocks;
  if (slice >= (size_t)A.slices) return;   // (the last workgroup's spare wavefronts; no workgroup-wide barrier below)
  size_t o = (wave_id % out_blocks) * IPW + grp;
  const bool live = o < A.n_out;
  if (!live) o = A.n_out - 1;
  // o = ((n * c_out + co) * oh + oy) * ow + ox; n_out = images of the tile * c_out * oh * ow: n stays inside the tile
  const uint32_t ox = (uint32_t)(o % A.ow), oy = (uint32_t)(o / A.ow % A.oh);
  const size_t nc = o / A.ow / A.oh;
  const uint32_t co = (uint32_t)(nc % A.c_out);
  const size_t img = nc / A.c_out;
  const int y0 = (int)(oy * A.sh) - (int)A.ph, x0 = (int)(ox * A.sw) - (int)A.pw;   // the window's corner, may lie outside
  const uint32_t kk = A.kh * A.kw, taps = A.c_in * kk;
  const uint32_t lo = (uint32_t)((uint64_t)slice * taps / (uint32_t)A.slices),
                 hi = (uint32_t)((uint64_t)(slice + 1) * taps / (uint32_t)A.slices);   // slices <= taps: never empty
  const uint32_t lo_ci = lo / kk, lo_ky = lo % kk / A.kw, lo_kx = lo % A.kw;            // the only divisions of the walk
  uint32_t n[K], a[K], b[K], ma[K], mb[K];
#pragma unroll
  for (int j = 0; j < K; ++j) n[j] = A.ctx.nhat[x * K + j];
  const int w = A.window, trows = (1 << w) + 1;
  const int nwin = (A.e_bits + w - 1) / w;
  const int top_bits = A.e_bits - (nwin - 1) * w + 1;
  const uint64_t* wrow = A.wt + (size_t)co * taps * A.w_stride;
  const uint32_t* timg = A.table + img * A.c_in * A.h * A.w * (size_t)trows * LQ;
  auto inside = [&](const ConvPos& p) -> bool {
    const int iy = y0 + (int)p.ky, ix = x0 + (int)p.kx;
    return iy >= 0 && iy < (int)A.h && ix >= 0 && ix < (int)A.w;
  };
  // the table row of a position; row 0 for a tap outside the image, whatever its weight's sign
  auto digit = [&](const ConvPos& p) -> int {
    const int d = signed_digit_row(wrow + (size_t)p.tap * A.w_stride, A.w_words, w, p.win, nwin, top_bits);
    return inside(p) ? d : 0;
  };
  // the entry of a position: the tap's element, clamped into the image (a clamped tap comes with row 0)
  auto load_entry = [&](uint32_t (&da)[K], uint32_t (&db)[K], const ConvPos& p, int d) {
    int iy = y0 + (int)p.ky, ix = x0 + (int)p.kx;
    iy = iy < 0 ? 0 : (iy >= (int)A.h ? (int)A.h - 1 : iy);
    ix = ix < 0 ? 0 : (ix >= (int)A.w ? (int)A.w - 1 : ix);
    const size_t elem = ((size_t)p.ci * A.h + (size_t)iy) * A.w + (size_t)ix;
    const uint32_t* e = timg + (elem * (size_t)trows + (size_t)d) * LQ;
    load_pair_row<K>(da, e, x);
    load_pair_row<K>(db, e + L2, x);
  };
  // positions (win, tap) in the order the schedule visits them: the top window's taps, then window by window down
  auto advance = [&](ConvPos& p) {
    if (++p.tap == hi) {
      p.tap = lo;
      p.ci = lo_ci;
      p.ky = lo_ky;
      p.kx = lo_kx;
      --p.win;
    } else if (++p.kx == A.kw) {
      p.kx = 0;
      if (++p.ky == A.kh) {
        p.ky = 0;
        ++p.ci;
      }
    }
  };
  // as in conv_kernel: the accumulator starts as the entry of the first position (the top window needs no squarings);
  // (ma, mb) holds the entry of the position about to be multiplied in, dn the row of the one after it
  ConvPos c{lo, lo_ci, lo_ky, lo_kx, nwin - 1}, nx;
  load_entry(a, b, c, digit(c));
  advance(c);
  if (c.win >= 0) load_entry(ma, mb, c, digit(c));
  nx = c;
  int dn = 0;
  if (nx.win >= 0) {
    advance(nx);
    if (nx.win >= 0) dn = digit(nx);
  }
#pragma unroll 1
  while (c.win >= 0) {
    uint32_t na[K], nb[K];
    ConvPos f = nx;
    if (nx.win >= 0) {
      load_entry(na, nb, nx, dn);
      advance(f);
      if (f.win >= 0) dn = digit(f);
    }
    if (c.tap == lo) {   // first tap of a window below the top one
#pragma unroll 1
      for (int i = 0; i < w; ++i) seq_pairmul<G, K, true, true, true>(a, b, a, b, n, 0, sel0, qs, ts);
    }
    // (a zero digit, a padded tap's included, multiplies by row 0 = one: no branch around a product that exchanges data
    // across the group)
    seq_pairmul<G, K, false, true, true>(a, b, ma, mb, n, 0, sel0, qs, ts);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      ma[j] = na[j];
      mb[j] = nb[j];
    }
    c = nx;
    nx = f;
  }
  if (live) {
    uint32_t* out = A.out + (slice * A.o_slice_stride + o) * (size_t)LQ;
    store_pair_row<K>(out, a, x);
    store_pair_row<K>(out + L2, b, x);
  }
}

}  // namespace pgpu

#endif  // PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_CONV_SIGNED_HPP_
