// pailliercryptolib_amd -- the encrypted segmented prefix sum on resident ciphertexts (pgpu_batch_ct_segment_scan):
//     out[r][t] = prod_{ u <= t } X[r][u]  mod n^2     (reverse: u >= t)      the cumulative sums under the encryption
// x is read as [rows][seg_len].  A row of at most `chunk` entries is one product chain; a longer row is cut into chunks
// and scanned by reduce-then-scan (policy.cpp: segscan_plan): segsum_kernel multiplies every chunk but the last of a row
// into a total, the totals -- [rows][chunks - 1] -- are scanned by the same procedure, and this kernel walks every chunk
// once more, starting from the scanned total of the chunks before it, and stores the running product after every entry.
// The schedule is restated in plain integers in tests/test_segscan_model.py.
//
// The arithmetic is seq_pairmul of hensel_seq.hpp, lazily reduced: the rows this kernel and segsum_kernel store are valid
// operands on both sides of the next product, so nothing is reduced between the steps or between the levels.  The rows
// are addressed by arithmetic on rows, seg_len and the plan alone: no index list, nothing that depends on a value.
#ifndef PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_SEGSCAN_HPP_
#define PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_SEGSCAN_HPP_

#include "hensel_seq.hpp"

namespace pgpu {

// One wavefront = 64/G chunks.  A chain that starts from a carry row multiplies all len entries in; one without starts as
// entry 0 (stored unchanged) and multiplies len - 1.  The trip count is the most products any chain of the wavefront
// has; a group past its own end multiplies by the row of one and stores nothing.
template <int G, int K>
__global__ __launch_bounds__(kWGThreads, 2) void segscan_kernel(SegscanArgs A) {
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
  if (!live) ci = A.n_chunks - 1;   // (idle groups of the last wavefront walk a valid chunk -- the shortest -- and do not store)
  const SegscanChunk c = A.chunks[ci];
  const uint32_t len = c.len;
  const bool carried = c.carry != kSegscanNoCarry;
  const uint32_t first = carried ? 0u : 1u;   // the first entry that is multiplied in
  // the most products of any chain of the wavefront, in a scalar register: the loop below is the same for every group
  uint32_t longest = len - first;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) longest = max(longest, (uint32_t)__shfl_xor((int)longest, d, kWave));
  longest = (uint32_t)__builtin_amdgcn_readfirstlane((int)longest);
  uint32_t n[K], a[K], b[K], ma[K], mb[K];
#pragma unroll
  for (int j = 0; j < K; ++j) n[j] = A.ctx.nhat[x * K + j];
  // entry t of the chain as a row number of src and out: begin + t or begin - t
  const ptrdiff_t step = A.step;
  auto index_of = [&](uint32_t t) -> size_t { return (size_t)c.begin + (size_t)(step * (ptrdiff_t)t); };
  // no load hangs on a condition: past the end the row is the row of one -- a select between two addresses, not a branch
  // around a load
  auto row_of = [&](uint32_t t) -> const uint32_t* { return t < len ? A.src + index_of(t) * (size_t)LQ : A.ctx.one; };
  auto load_row = [&](uint32_t (&da)[K], uint32_t (&db)[K], const uint32_t* row) {
    load_pair_row<K>(da, row, x);
    load_pair_row<K>(db, row + L2, x);
  };
  auto store_row = [&](uint32_t t) {
    uint32_t* o = A.out + index_of(t) * (size_t)LQ;
    store_pair_row<K>(o, a, x);
    store_pair_row<K>(o + L2, b, x);
  };
  // the accumulator starts as the carry row, or as entry 0; (ma, mb) holds the entry about to be multiplied in: a row's
  // load travels while the product before it runs
  load_row(a, b, carried ? A.carry + (size_t)c.carry * (size_t)LQ : A.src + (size_t)c.begin * (size_t)LQ);
  load_row(ma, mb, row_of(first));
  if (!carried && live) store_row(0);
#pragma unroll 1
  for (uint32_t i = 0; i < longest; ++i) {
    const uint32_t t = first + i;
    uint32_t na[K], nb[K];
    load_row(na, nb, row_of(t + 1));
    // (no branch on a length around a product that exchanges data across the group; the store is per lane and may have one)
    seq_pairmul<G, K, false, true, true>(a, b, ma, mb, n, 0, sel0, qs, ts);
    if (t < len && live) store_row(t);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      ma[j] = na[j];
      mb[j] = nb[j];
    }
  }
}

}  // namespace pgpu

#endif  // PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_SEGSCAN_HPP_
