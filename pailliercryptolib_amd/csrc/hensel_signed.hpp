// pailliercryptolib_amd -- the signed-weight encrypted matrix-vector and matrix products on resident ciphertexts
// (pgpu_batch_ct_matvec_signed / pgpu_batch_ct_matmul_signed):
//     Y[i] = prod_j X[j]^W[i][j]  mod n^2,   W[i][j] a SIGNED integer, two's complement in e_bits bits.
// With X[j]^-1 resident (the batched inversion of hensel_invert.hpp, run by the host before the first launch here) a
// signed weight costs no more products than an unsigned one: the weight is recoded into radix-2^w Booth digits
//     d_k = -2^(w-1) b[kw+w-1] + sum_{i<w-1} 2^i b[kw+i] + b[kw-1],     b[-1] = 0,  b[i] = b[e_bits-1] for i >= e_bits,
// k = 0 .. nwin - 1, nwin = ceil(e_bits / w): d_k in [-h, h] with h = 2^(w-1), and sum d_k 2^(kw) = W.  A digit depends on
// w + 1 neighbouring bits alone -- no carry chain -- so the top-down walk cuts it on the fly, across 64-bit words.  The table
// of an element holds 2h + 1 rows, as many products to build as the 2^w rows of the unsigned one:
//     row 0 = one,   rows 1 .. h = x^1 .. x^h,   rows h+1 .. 2h = x^-1 .. x^-h,
// and digit d selects row d (d >= 0) or row h - d (d < 0).
//   * matvec_signed_table_kernel: one group of G lanes per (element, half); half 0 walks x, half 1 walks x^-1, each the
//     loop of matvec_table_kernel over h - 1 products;
//   * matvec_signed_kernel / matmul_signed_kernel: the schedules of matvec_kernel / matmul_kernel (hensel_matvec.hpp,
//     hensel_matmul.hpp) -- top-down windows, w squarings per window, one product per column, the two-ahead digit fetch
//     and one-ahead entry load, wavefront-uniform slices, dead groups clamped and not stored -- with the digit cut and the
//     row selection above in place of theirs.
// The schedule is restated in plain integers in tests/test_signed_matvec_model.py; w, the slices and the tile are host
// policy (policy.cpp: matvec_signed_window, matmul_signed_plan).
//
// The arithmetic is seq_pairmul of hensel_seq.hpp on pair rows.  The table is indexed by digits of the caller's PLAINTEXT
// matrix (the indexed access of the default table_gather_policy; the host refuses the call under the masked policy).
#ifndef PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_SIGNED_HPP_
#define PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_SIGNED_HPP_

#include "hensel_seq.hpp"

namespace pgpu {

// The table row that window `win` of the weight at `ep` selects.  top_bits = e_bits - (nwin - 1) * w + 1: the bits of the
// top window's cut (its look-behind bit included) that lie below e_bits; what lies above them is the sign, whatever the
// stored words hold there.  Only the top window reaches e_bits: (win + 1) * w <= (nwin - 1) * w < e_bits below it.
__device__ __forceinline__ int signed_digit_row(const uint64_t* ep, int w_words, int w, int win, int nwin, int top_bits) {
  uint64_t u;
  if (win == 0) {
    u = ep[0] << 1;                                   // b[-1] = 0
  } else {
    const int bit = win * w - 1;                      // the look-behind bit: < e_bits <= 64 * w_words
    const int word = bit >> 6, sh = bit & 63;
    u = ep[word] >> sh;
    if (sh + w + 1 > 64 && word + 1 < w_words) u |= ep[word + 1] << (64 - sh);
  }
  if (win == nwin - 1) u = (uint64_t)((int64_t)(u << (64 - top_bits)) >> (64 - top_bits));   // sign-extend (top_bits <= w + 1)
  const int h = 1 << (w - 1);
  const int c = (int)(u & (uint64_t)(2 * h - 1));     // b[kw-1], b[kw] .. b[kw+w-2]
  const int d = (c >> 1) + (c & 1) - (int)((u >> w) & 1) * h;
  return d >= 0 ? d : h - d;
}

// T[e][.] over [x_e ; x_e^-1] as pair rows: row 0 = one; rows 1..h = x^1..x^h (half 0); rows h+1..2h = x^-1..x^-h (half 1).
// Group 2e + half of the launch handles (e, half): row r0 + 1 is its base, row r0 + d row r0 + d - 1 times the base.
template <int G, int K>
__global__ __launch_bounds__(kWGThreads, 2) void matvec_signed_table_kernel(SignedTableArgs A) {
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
  size_t item = ((size_t)blockIdx.x * kWavesPerWG + wv) * IPW + grp;
  const bool live = item < 2 * A.elems;
  if (!live) item = 2 * A.elems - 1;
  const size_t el = item >> 1;
  const bool inv = (item & 1) != 0;
  uint32_t n[K], a[K], b[K], ma[K], mb[K];
#pragma unroll
  for (int j = 0; j < K; ++j) n[j] = A.ctx.nhat[x * K + j];
  const int h = 1 << (A.window - 1);
  uint32_t* tbl = A.table + el * (size_t)(2 * h + 1) * LQ;
  {
    const uint32_t* row = (inv ? A.xinv : A.x) + el * (size_t)LQ;
    load_pair_row<K>(a, row, x);
    load_pair_row<K>(b, row + L2, x);
  }
  if (live && !inv) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      ma[j] = A.ctx.one[x * K + j];
      mb[j] = A.ctx.one[L2 + x * K + j];
    }
    store_pair_row<K>(tbl, ma, x);
    store_pair_row<K>(tbl + L2, mb, x);
  }
  tbl += (inv ? (size_t)h : 0) * LQ;      // row d of this half: tbl + d * LQ, d = 1 .. h
  if (live) {
    store_pair_row<K>(tbl + LQ, a, x);
    store_pair_row<K>(tbl + LQ + L2, b, x);
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    ma[j] = a[j];
    mb[j] = b[j];
  }
#pragma unroll 1
  for (int e = 2; e <= h; ++e) {
    seq_pairmul<G, K, false, true, true>(a, b, ma, mb, n, 0, sel0, qs, ts);
    if (live) {
      store_pair_row<K>(tbl + (size_t)e * LQ, a, x);
      store_pair_row<K>(tbl + (size_t)e * LQ + L2, b, x);
    }
  }
}

// matvec_kernel on Booth digits: one wavefront = 64/G rows of ONE column slice; partial products leave as pair rows
// out[slice][row].
template <int G, int K>
__global__ __launch_bounds__(kWGThreads, 2) void matvec_signed_kernel(MatvecArgs A) {
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
  const size_t row_blocks = (A.rows + IPW - 1) / IPW;
  const size_t slice = wave_id / row_blocks;
  if (slice >= (size_t)A.slices) return;   // (the last workgroup's spare wavefronts; no workgroup-wide barrier below)
  size_t row = (wave_id % row_blocks) * IPW + grp;
  const bool live = row < A.rows;
  if (!live) row = A.rows - 1;
  const size_t lo = slice * A.cols / (size_t)A.slices, hi = (slice + 1) * A.cols / (size_t)A.slices;   // slices <= cols: never empty
  uint32_t n[K], a[K], b[K], ma[K], mb[K];
#pragma unroll
  for (int j = 0; j < K; ++j) n[j] = A.ctx.nhat[x * K + j];
  const int w = A.window, trows = (1 << w) + 1;
  const int nwin = (A.e_bits + w - 1) / w;
  const int top_bits = A.e_bits - (nwin - 1) * w + 1;
  const uint64_t* wrow = A.w + row * A.cols * A.w_stride;
  auto digit = [&](size_t j, int win) -> int {
    return signed_digit_row(wrow + j * A.w_stride, A.w_words, w, win, nwin, top_bits);
  };
  auto load_entry = [&](uint32_t (&da)[K], uint32_t (&db)[K], size_t j, int d) {
    const uint32_t* e = A.table + (j * (size_t)trows + (size_t)d) * LQ;
    load_pair_row<K>(da, e, x);
    load_pair_row<K>(db, e + L2, x);
  };
  // positions (win, j) in the order the schedule visits them: the top window's columns, then window by window down
  auto advance = [&](size_t& j, int& win) {
    if (++j == hi) {
      j = lo;
      --win;
    }
  };
  // as in matvec_kernel: the accumulator starts as the entry of the first position (the top window needs no squarings);
  // (ma, mb) holds the entry of the position about to be multiplied in, dn the row of the one after it
  size_t cj = lo, nj;
  int cwin = nwin - 1, nw;
  load_entry(a, b, cj, digit(cj, cwin));
  advance(cj, cwin);
  if (cwin >= 0) load_entry(ma, mb, cj, digit(cj, cwin));
  nj = cj;
  nw = cwin;
  int dn = 0;
  if (nw >= 0) {
    advance(nj, nw);
    if (nw >= 0) dn = digit(nj, nw);
  }
#pragma unroll 1
  while (cwin >= 0) {
    uint32_t na[K], nb[K];
    size_t fj = nj;
    int fw = nw;
    if (nw >= 0) {
      load_entry(na, nb, nj, dn);
      advance(fj, fw);
      if (fw >= 0) dn = digit(fj, fw);
    }
    if (cj == lo) {   // first column of a window below the top one
#pragma unroll 1
      for (int i = 0; i < w; ++i) seq_pairmul<G, K, true, true, true>(a, b, a, b, n, 0, sel0, qs, ts);
    }
    // (a zero digit multiplies by row 0 = one: no branch on a digit around a product that exchanges data across the group)
    seq_pairmul<G, K, false, true, true>(a, b, ma, mb, n, 0, sel0, qs, ts);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      ma[j] = na[j];
      mb[j] = nb[j];
    }
    cj = nj;
    cwin = nw;
    nj = fj;
    nw = fw;
  }
  if (live) {
    uint32_t* out = A.out + (slice * A.rows + row) * (size_t)LQ;
    store_pair_row<K>(out, a, x);
    store_pair_row<K>(out + L2, b, x);
  }
}

// matmul_kernel on Booth digits: one wavefront = 64/G consecutive outputs o = v * rows + i of ONE column slice; the table
// strides count elements of 2h + 1 rows.
template <int G, int K>
__global__ __launch_bounds__(kWGThreads, 2) void matmul_signed_kernel(MatmulArgs A) {
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
  const size_t v = o / A.rows, row = o % A.rows;   // n_out = vectors of the tile * rows: v stays inside the tile
  const size_t lo = slice * A.cols / (size_t)A.slices, hi = (slice + 1) * A.cols / (size_t)A.slices;   // slices <= cols: never empty
  uint32_t n[K], a[K], b[K], ma[K], mb[K];
#pragma unroll
  for (int j = 0; j < K; ++j) n[j] = A.ctx.nhat[x * K + j];
  const int w = A.window, trows = (1 << w) + 1;
  const int nwin = (A.e_bits + w - 1) / w;
  const int top_bits = A.e_bits - (nwin - 1) * w + 1;
  const uint64_t* wrow = A.w + row * A.cols * A.w_stride;
  const uint32_t* tvec = A.table + v * A.t_vec_stride * (size_t)trows * LQ;
  const size_t tcol = A.t_col_stride * (size_t)trows * LQ;
  auto digit = [&](size_t j, int win) -> int {
    return signed_digit_row(wrow + j * A.w_stride, A.w_words, w, win, nwin, top_bits);
  };
  auto load_entry = [&](uint32_t (&da)[K], uint32_t (&db)[K], size_t j, int d) {
    const uint32_t* e = tvec + j * tcol + (size_t)d * LQ;
    load_pair_row<K>(da, e, x);
    load_pair_row<K>(db, e + L2, x);
  };
  // positions (win, j) in the order the schedule visits them: the top window's columns, then window by window down
  auto advance = [&](size_t& j, int& win) {
    if (++j == hi) {
      j = lo;
      --win;
    }
  };
  // as in matmul_kernel: the accumulator starts as the entry of the first position; (ma, mb) holds the entry of the position
  // about to be multiplied in, dn the row of the one after it
  size_t cj = lo, nj;
  int cwin = nwin - 1, nw;
  load_entry(a, b, cj, digit(cj, cwin));
  advance(cj, cwin);
  if (cwin >= 0) load_entry(ma, mb, cj, digit(cj, cwin));
  nj = cj;
  nw = cwin;
  int dn = 0;
  if (nw >= 0) {
    advance(nj, nw);
    if (nw >= 0) dn = digit(nj, nw);
  }
#pragma unroll 1
  while (cwin >= 0) {
    uint32_t na[K], nb[K];
    size_t fj = nj;
    int fw = nw;
    if (nw >= 0) {
      load_entry(na, nb, nj, dn);
      advance(fj, fw);
      if (fw >= 0) dn = digit(fj, fw);
    }
    if (cj == lo) {   // first column of a window below the top one
#pragma unroll 1
      for (int i = 0; i < w; ++i) seq_pairmul<G, K, true, true, true>(a, b, a, b, n, 0, sel0, qs, ts);
    }
    // (a zero digit multiplies by row 0 = one: no branch on a digit around a product that exchanges data across the group)
    seq_pairmul<G, K, false, true, true>(a, b, ma, mb, n, 0, sel0, qs, ts);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      ma[j] = na[j];
      mb[j] = nb[j];
    }
    cj = nj;
    cwin = nw;
    nj = fj;
    nw = fw;
  }
  if (live) {
    uint32_t* out = A.out + (slice * A.o_slice_stride + v * A.o_vec_stride + row * A.o_row_stride) * (size_t)LQ;
    store_pair_row<K>(out, a, x);
    store_pair_row<K>(out + L2, b, x);
  }
}

}  // namespace pgpu

#endif  // PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_SIGNED_HPP_
