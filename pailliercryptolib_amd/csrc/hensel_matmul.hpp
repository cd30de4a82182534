// pailliercryptolib_amd -- the encrypted matrix product on resident ciphertexts (pgpu_batch_ct_matmul):
//     Y[v][i] = prod_j X[v][j]^W[i][j]  mod n^2      (Y = X*W^T under the encryption: a linear layer applied to n_vec vectors)
// The matvec of hensel_matvec.hpp for a TILE of vectors at a time:
//   * the window tables T[e][d] = x_e^d of the tile's elements are built by the unchanged matvec_table_kernel over the
//     tile's contiguous range of x (the host walks the vectors tile by tile and reuses one table block: policy.cpp:
//     matmul_plan);
//   * one group of G lanes per output (v, i) of the tile and column slice; the outputs are numbered flat, o = v * rows + i,
//     across the groups of a wavefront: a wavefront may straddle vectors, and only the last wavefront of a slice has dead
//     groups.  The schedule of an output is matvec_kernel's: from the top window down, w squarings, then one product per
//     column with T[element (v, j)][digit(W[i][j], win)];
//   * where an element (v, j) sits in the table and where an output (v, i) is stored are two strides each
//     (t_vec_stride / t_col_stride, o_vec_stride / o_row_stride): x read as [n_vec][cols] or as [cols][n_vec] is the same
//     instruction stream.  The weight digit depends on i alone.
// The schedule is restated in plain integers in tests/test_matmul_model.py.
//
// The arithmetic is seq_pairmul of hensel_seq.hpp on pair rows.  The table is indexed by digits of the caller's PLAINTEXT
// matrix (the indexed access of the default table_gather_policy; the host refuses the call under the masked policy).
#ifndef PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_MATMUL_HPP_
#define PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_MATMUL_HPP_

#include "hensel_seq.hpp"

namespace pgpu {

// One wavefront = 64/G consecutive outputs of ONE column slice (slice and column range are wavefront-uniform: every group
// of the wavefront walks the same columns and windows, only the table rows and the digits differ).
template <int G, int K>
__global__ __launch_bounds__(kWGThreads, 2) void matmul_kernel(MatmulArgs A) {
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
  const int w = A.window, tsize = 1 << w;
  const int nwin = (A.e_bits + w - 1) / w;
  const uint64_t top_mask = ((uint64_t)1 << (A.e_bits - (nwin - 1) * w)) - 1;   // bits of the top window below e_bits
  const uint64_t* wrow = A.w + row * A.cols * A.w_stride;
  const uint32_t* tvec = A.table + v * A.t_vec_stride * (size_t)tsize * LQ;
  const size_t tcol = A.t_col_stride * (size_t)tsize * LQ;
  auto digit = [&](size_t j, int win) -> int {
    const uint64_t* ep = wrow + j * A.w_stride;
    const int bit = win * w;
    const int word = bit >> 6, sh = bit & 63;
    uint64_t d = (word < A.w_words) ? ep[word] >> sh : 0;
    if (sh + w > 64 && word + 1 < A.w_words) d |= ep[word + 1] << (64 - sh);
    if (win == nwin - 1) d &= top_mask;
    return (int)(d & (uint64_t)(tsize - 1));
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
  // as in matvec_kernel: the accumulator starts as the entry of the first position (the top window needs no squarings);
  // (ma, mb) holds the entry of the position about to be multiplied in, dn the digit of the one after it
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
    // (a zero digit multiplies by T[.][0] = one: no branch on a digit around a product that exchanges data across the group)
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

#endif  // PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_MATMUL_HPP_
