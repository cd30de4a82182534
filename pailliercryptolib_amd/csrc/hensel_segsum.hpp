// pailliercryptolib_amd -- the encrypted segmented sum on resident ciphertexts (pgpu_batch_ct_segment_sum):
//     out[g][s] = prod_{ j : ids[g][j] == s } X[j]  mod n^2          (a histogram / grouped aggregate under the encryption)
// The host sorts the element numbers of every group by segment (policy.cpp: segsum_sort), cuts every segment into chunks
// of at most `chunk` consecutive entries and hands the kernel one descriptor {begin, len, dst} per chunk (segsum_plan).
// One group of G lanes multiplies the rows of one chunk into one row; a segment of several chunks leaves partial rows,
// which the same kernel folds in the next level (perm == null: the identity), the last level of every segment straight
// into the result batch.  The schedule is restated in plain integers in tests/test_segsum_model.py.
//
// The arithmetic is seq_pairmul of hensel_seq.hpp, lazily reduced: a chain of any length needs no reduction in between,
// and pair rows are multiplied as they lie in memory.  The rows are addressed by the caller's PLAINTEXT segment ids (the
// indexed access of the default table_gather_policy; the host refuses the call under the masked policy).
#ifndef PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_SEGSUM_HPP_
#define PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_SEGSUM_HPP_

#include "hensel_seq.hpp"

namespace pgpu {

// One wavefront = 64/G chunks.  The trip count is the longest chunk of the wavefront (the descriptors arrive ordered by
// length, so the chunks of a wavefront are nearly equally long); a group past its own end multiplies by the row of one.
template <int G, int K>
__global__ __launch_bounds__(kWGThreads, 2) void segsum_kernel(SegsumArgs A) {
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
  const SegsumChunk c = A.chunks[ci];
  const uint32_t len = c.len;
  // the longest chunk of the wavefront, in a scalar register: the loop below is the same for every group
  uint32_t longest = len;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) longest = max(longest, (uint32_t)__shfl_xor((int)longest, d, kWave));
  longest = (uint32_t)__builtin_amdgcn_readfirstlane((int)longest);
  uint32_t n[K], a[K], b[K], ma[K], mb[K];
#pragma unroll
  for (int j = 0; j < K; ++j) n[j] = A.ctx.nhat[x * K + j];
  // entry t of the chunk as an element number and as a row.  Neither load hangs on a condition: past the end the entry
  // read is entry 0 of the list (the host keeps at least one there) and the row is the row of one -- a select between two
  // addresses, not a branch around a load.
  const bool ident = A.perm == nullptr;
  auto index_of = [&](uint32_t t) -> size_t {
    const size_t pos = t < len ? (size_t)c.begin + t : 0;
    return ident ? pos : (size_t)A.perm[pos];
  };
  auto row_of = [&](uint32_t t, size_t idx) -> const uint32_t* { return t < len ? A.src + idx * (size_t)LQ : A.ctx.one; };
  auto load_row = [&](uint32_t (&da)[K], uint32_t (&db)[K], const uint32_t* row) {
    load_pair_row<K>(da, row, x);
    load_pair_row<K>(db, row + L2, x);
  };
  // the accumulator starts as entry 0 (an empty chunk: one); (ma, mb) holds the entry about to be multiplied in, inext
  // the element number of the one after it: a row's load travels while the product before it runs, and its index -- the
  // load the row's address hangs on -- was fetched a product earlier still
  load_row(a, b, row_of(0, index_of(0)));
  load_row(ma, mb, row_of(1, index_of(1)));
  size_t inext = index_of(2);
#pragma unroll 1
  for (uint32_t t = 1; t < longest; ++t) {
    uint32_t na[K], nb[K];
    load_row(na, nb, row_of(t + 1, inext));
    inext = index_of(t + 2);
    // (no branch on a length around a product that exchanges data across the group)
    seq_pairmul<G, K, false, true, true>(a, b, ma, mb, n, 0, sel0, qs, ts);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      ma[j] = na[j];
      mb[j] = nb[j];
    }
  }
  if (live) {
    uint32_t* out = ((c.dst & kSegsumPartial) ? A.partial : A.out) + (size_t)(c.dst & ~kSegsumPartial) * LQ;
    store_pair_row<K>(out, a, x);
    store_pair_row<K>(out + L2, b, x);
  }
}

}  // namespace pgpu

#endif  // PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_SEGSUM_HPP_
