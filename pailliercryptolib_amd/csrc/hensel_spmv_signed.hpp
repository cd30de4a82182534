// pailliercryptolib_amd -- the signed-weight encrypted sparse matrix-vector product on resident ciphertexts
// (pgpu_batch_ct_spmv_signed):
//     out[i] = prod_{ row_ptr[i] <= t < row_ptr[i+1] } X[col_idx[t]]^w[t]  mod n^2,   w[t] a SIGNED integer, two's complement
// in e_bits bits.  spmv_kernel of hensel_spmv.hpp on the tables and digits of hensel_signed.hpp:
//   * the tables T[j][.] over [X[j] ; X[j]^-1] -- 2^w + 1 rows per column: row 0 = one, rows 1..h = x^1..x^h, rows h+1..2h =
//     x^-1..x^-h, h = 2^(w-1) -- are built once per call by the unchanged matvec_signed_table_kernel over ALL columns of x
//     (the host inverts all of x before);
//   * the chains, their descriptors and the schedule are spmv_kernel's, unchanged: one group of G lanes per chain, from the
//     top window down w squarings and one product per entry, the trip count of a wavefront its longest chain, the fold of
//     the partial rows by segsum_kernel in the levels after;
//   * the row of an entry is signed_digit_row of its weight's Booth digit (row d, or row h - d for d < 0), and the table
//     stride counts columns of 2^w + 1 rows;
//   * a position past the chain's end still reads CSR position 0 and multiplies by the row of one: a select between two
//     addresses, not a branch around a load.
// The schedule is restated in plain integers in tests/test_spmv_signed_model.py.
//
// The arithmetic is seq_pairmul of hensel_seq.hpp, lazily reduced.  The table is indexed by the caller's PLAINTEXT column
// numbers and by digits of the caller's PLAINTEXT weights, never by key material or anything encrypted (the indexed
// access of the default table_gather_policy; the host refuses the call under the masked policy).
#ifndef PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_SPMV_SIGNED_HPP_
#define PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_SPMV_SIGNED_HPP_

#include "hensel_signed.hpp"    // signed_digit_row

namespace pgpu {

// One wavefront = 64/G chains, as in spmv_kernel.
template <int G, int K>
__global__ __launch_bounds__(kWGThreads, 2) void spmv_signed_kernel(SpmvArgs A) {
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
  size_t ci = ((size_t)blockIdx.x * kWavesPerWG + wv) * IPW + grp;
  const bool live = ci < A.n_chunks;
  if (!live) ci = A.n_chunks - 1;   // (idle groups of the last wavefront walk a valid chain -- the shortest -- and do not store)
  const SegsumChunk c = A.chunks[ci];
  const uint32_t len = c.len;
  // the longest chain of the wavefront, in a scalar register: the loop below is the same for every group.  At least 1:
  // a wavefront of empty rows walks one position per window, every entry of it the row of one.
  uint32_t longest = len;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) longest = max(longest, (uint32_t)__shfl_xor((int)longest, d, kWave));
  longest = max((uint32_t)__builtin_amdgcn_readfirstlane((int)longest), 1u);
  uint32_t n[K], a[K], b[K], ma[K], mb[K];
#pragma unroll
  for (int j = 0; j < K; ++j) n[j] = A.ctx.nhat[x * K + j];
  const int w = A.window, trows = (1 << w) + 1;
  const int nwin = (A.e_bits + w - 1) / w;
  const int top_bits = A.e_bits - (nwin - 1) * w + 1;
  // the table entry of position (win, t) as an address.  Neither the column index nor the digit hangs on a condition: past
  // the chain's end both are read at CSR position 0 (the host keeps at least one entry there) and the entry is the row of
  // one -- a select between two addresses, not a branch around a load.
  auto entry_of = [&](uint32_t t, int win) -> const uint32_t* {
    const bool in = t < len;
    const size_t pos = in ? (size_t)c.begin + t : 0;
    const size_t col = A.col_idx[pos];
    const int d = signed_digit_row(A.w + pos * A.w_stride, A.w_words, w, win, nwin, top_bits);
    const uint32_t* e = A.table + (col * (size_t)trows + (size_t)d) * LQ;
    return in ? e : A.ctx.one;
  };
  auto load_entry = [&](uint32_t (&da)[K], uint32_t (&db)[K], const uint32_t* e) {
    load_pair_row<K>(da, e, x);
    load_pair_row<K>(db, e + L2, x);
  };
  // positions (win, t) in the order the schedule visits them: the top window's entries, then window by window down
  auto advance = [&](uint32_t& t, int& win) {
    if (++t == longest) {
      t = 0;
      --win;
    }
  };
  // as in spmv_kernel: the accumulator starts as the entry of the first position (the top window needs no squarings);
  // (ma, mb) holds the entry of the position about to be multiplied in, en the address of the one after it
  uint32_t ct = 0, nt;
  int cwin = nwin - 1, nw;
  load_entry(a, b, entry_of(ct, cwin));
  advance(ct, cwin);
  if (cwin >= 0) load_entry(ma, mb, entry_of(ct, cwin));
  nt = ct;
  nw = cwin;
  const uint32_t* en = A.ctx.one;
  if (nw >= 0) {
    advance(nt, nw);
    if (nw >= 0) en = entry_of(nt, nw);
  }
#pragma unroll 1
  while (cwin >= 0) {
    uint32_t na[K], nb[K];
    uint32_t ft = nt;
    int fw = nw;
    if (nw >= 0) {
      load_entry(na, nb, en);
      advance(ft, fw);
      if (fw >= 0) en = entry_of(ft, fw);
    }
    if (ct == 0) {   // first entry of a window below the top one
#pragma unroll 1
      for (int i = 0; i < w; ++i) seq_pairmul<G, K, true, true, true>(a, b, a, b, n, 0, sel0, qs, ts);
    }
    // (a zero digit multiplies by row 0 = one, an entry past the chain's end by the row of one: no branch on a digit or a
    // length around a product that exchanges data across the group)
    seq_pairmul<G, K, false, true, true>(a, b, ma, mb, n, 0, sel0, qs, ts);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      ma[j] = na[j];
      mb[j] = nb[j];
    }
    ct = nt;
    cwin = nw;
    nt = ft;
    nw = fw;
  }
  if (live) {
    uint32_t* out = ((c.dst & kSegsumPartial) ? A.partial : A.out) + (size_t)(c.dst & ~kSegsumPartial) * LQ;
    store_pair_row<K>(out, a, x);
    store_pair_row<K>(out + L2, b, x);
  }
}

}  // namespace pgpu

#endif  // PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_SPMV_SIGNED_HPP_
