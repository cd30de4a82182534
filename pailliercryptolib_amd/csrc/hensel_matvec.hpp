// pailliercryptolib_amd -- the encrypted matrix-vector product on resident ciphertexts (pgpu_batch_ct_matvec):
//     Y[i] = prod_j X[j]^W[i][j]  mod n^2          (an encrypted linear layer: y = W*x under the encryption)
// as a simultaneous (Straus / interleaved fixed-window) multi-exponentiation on pair rows.  Composed from the
// element-wise operations a row costs cols exponentiations -- each with its own squaring chain and its own window
// table -- and cols - 1 products.  Here
//   * the window tables T[j][d] = X[j]^d, d = 0 .. 2^w - 1, are built ONCE per call (matvec_table_kernel: one group of
//     G lanes per column, the loop at the head of hensel_modexp_seq_kernel) and shared by all rows;
//   * the e_bits squarings are done once per OUTPUT (and column slice), not once per term (matvec_kernel: one group per
//     row and slice; from the top window down: w squarings, then one product per column with T[j][digit(W[i][j], win)]).
// The columns are cut into `slices` ranges so that a matrix of few rows still puts a wavefront on every SIMD; the
// partial products of a row are folded afterwards with element-wise pair products (capi_batches.inc).  The schedule is
// restated in plain integers in tests/test_matvec_model.py; w and the slice count are host policy (policy.cpp:
// matvec_plan).
//
// The arithmetic is seq_pairmul of hensel_seq.hpp (both halves of a pair in the same G lanes, quotient digits through
// LDS), the rows are the pair rows of kargs.hpp: a table entry is multipliable as it is.  The table is indexed by digits
// of the caller's PLAINTEXT matrix (the indexed access of the default table_gather_policy; the host refuses the call
// under the masked policy).
#ifndef PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_MATVEC_HPP_
#define PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_MATVEC_HPP_

#include "hensel_seq.hpp"

namespace pgpu {

// T[col][d] = X[col]^d as pair rows: entry 0 = one, entry 1 = the ciphertext, entry d = entry d-1 times the ciphertext
template <int G, int K>
__global__ __launch_bounds__(kWGThreads, 2) void matvec_table_kernel(MatvecArgs A) {
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
  size_t col = ((size_t)blockIdx.x * kWavesPerWG + wv) * IPW + grp;
  const bool live = col < A.cols;
  if (!live) col = A.cols - 1;
  uint32_t n[K], a[K], b[K], ma[K], mb[K];
#pragma unroll
  for (int j = 0; j < K; ++j) n[j] = A.ctx.nhat[x * K + j];
  const int tsize = 1 << A.window;
  uint32_t* tbl = A.table + col * (size_t)tsize * LQ;
  {
    const uint32_t* row = A.x + col * (size_t)LQ;
    load_pair_row<K>(a, row, x);
    load_pair_row<K>(b, row + L2, x);
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    ma[j] = A.ctx.one[x * K + j];
    mb[j] = A.ctx.one[L2 + x * K + j];
  }
  if (live) {
    store_pair_row<K>(tbl, ma, x);
    store_pair_row<K>(tbl + L2, mb, x);
    store_pair_row<K>(tbl + LQ, a, x);
    store_pair_row<K>(tbl + LQ + L2, b, x);
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    ma[j] = a[j];
    mb[j] = b[j];
  }
#pragma unroll 1
  for (int e = 2; e < tsize; ++e) {
    seq_pairmul<G, K, false, true, true>(a, b, ma, mb, n, 0, sel0, qs, ts);
    if (live) {
      store_pair_row<K>(tbl + (size_t)e * LQ, a, x);
      store_pair_row<K>(tbl + (size_t)e * LQ + L2, b, x);
    }
  }
}

// One wavefront = 64/G rows of ONE column slice (slice and column range are wavefront-uniform: every group of the
// wavefront walks the same columns and windows, only the digits -- the table entries -- differ).  Partial products
// leave as pair rows out[slice][row].
template <int G, int K>
__global__ __launch_bounds__(kWGThreads, 2) void matvec_kernel(MatvecArgs A) {
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
  const int w = A.window, tsize = 1 << w;
  const int nwin = (A.e_bits + w - 1) / w;
  const uint64_t top_mask = ((uint64_t)1 << (A.e_bits - (nwin - 1) * w)) - 1;   // bits of the top window below e_bits
  const uint64_t* wrow = A.w + row * A.cols * A.w_stride;
  auto digit = [&](size_t j, int win) -> int {
    const uint64_t* ep = wrow + j * A.w_stride;
    const int bit = win * w;
    const int word = bit >> 6, sh = bit & 63;
    uint64_t v = (word < A.w_words) ? ep[word] >> sh : 0;
    if (sh + w > 64 && word + 1 < A.w_words) v |= ep[word + 1] << (64 - sh);
    if (win == nwin - 1) v &= top_mask;
    return (int)(v & (uint64_t)(tsize - 1));
  };
  auto load_entry = [&](uint32_t (&da)[K], uint32_t (&db)[K], size_t j, int d) {
    const uint32_t* e = A.table + (j * (size_t)tsize + (size_t)d) * LQ;
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
  // the accumulator starts as the entry of the first position (the top window needs no squarings); (ma, mb) holds the
  // entry of the position about to be multiplied in, dn the digit of the one after it: an entry's load travels while the
  // product (and the squarings) before it run, and its digit was fetched a product earlier still
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
    // (a zero digit multiplies by T[j][0] = one: no branch on a digit around a product that exchanges data across the group)
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

}  // namespace pgpu

#endif  // PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_MATVEC_HPP_
