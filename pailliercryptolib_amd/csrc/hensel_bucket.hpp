// pailliercryptolib_amd -- the bucket reduction of the bucket-method encrypted matvec (pgpu_batch_ct_matvec_bucket):
//     S = prod_d B[d]^d  mod n^2      over the 2^c buckets of one (row, window)
// by running products, in two levels.  With block b (a power of two) and nb = 2^c / b:
//   level 1  one chain per block k:   U_k = prod_i B[k b + i],   V_k = prod_i B[k b + i]^i        (i = 0 .. b - 1)
//   level 2  one chain per window:    S = prod_k V_k * (prod_k U_k^k)^b
// Both are the same walk: from the last entry down to entry 1, acc <- acc * entry, tot <- tot * acc leaves
// tot = prod_i entry[i]^i (entry i is multiplied into acc i steps before the walk ends, and so enters tot i times).
// Level 1 then multiplies entry 0 into acc; level 2 squares tot log2 b times and multiplies the V_k in.  The schedule is
// restated in plain integers in tests/test_bucket_model.py.
//
// The arithmetic is seq_pairmul of hensel_seq.hpp, lazily reduced: nothing is reduced between the steps, and every row
// a chain stores comes out of a product or is an input row, so it is a valid operand on both sides of the next product
// anywhere.  The rows are addressed by arithmetic on the launch's sizes alone: no descriptors, no index list, nothing
// that depends on a value; every chain of a launch has the same trip count.
#ifndef PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_BUCKET_HPP_
#define PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_BUCKET_HPP_

#include "hensel_seq.hpp"

namespace pgpu {

// One wavefront = 64/G chains.  (a, b) is acc, (ta, tb) is tot, (ma, mb) holds the entry about to be multiplied in: its
// load is issued right after the first product of a step and travels under the second -- no third staged row.
template <int G, int K>
__global__ __launch_bounds__(kWGThreads, 2) void bucket_reduce_kernel(BucketArgs A) {
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
  size_t ch = ((size_t)blockIdx.x * kWavesPerWG + wv) * IPW + grp;
  const bool live = ch < A.chains;
  if (!live) ch = A.chains - 1;   // (idle groups of the last wavefront walk a valid chain and do not store)
  const uint32_t len = A.len, n_sqr = A.n_sqr, n_mul = A.n_mul;
  const uint32_t* row = A.src + ch * (size_t)len * (size_t)LQ;
  uint32_t n[K], a[K], b[K], ta[K], tb[K], ma[K], mb[K];
#pragma unroll
  for (int j = 0; j < K; ++j) n[j] = A.ctx.nhat[x * K + j];
  auto load_row = [&](uint32_t (&da)[K], uint32_t (&db)[K], const uint32_t* e) {
    load_pair_row<K>(da, e, x);
    load_pair_row<K>(db, e + L2, x);
  };
  // acc and tot start as the last entry (no product by a one); no load hangs on a condition: the step that multiplies
  // entry i in fetches entry i - 1, and the walk ends with entry 0 staged
  load_row(a, b, row + (size_t)(len - 1) * (size_t)LQ);
  load_row(ma, mb, row + (size_t)(len > 1 ? len - 2 : 0) * (size_t)LQ);
#pragma unroll
  for (int j = 0; j < K; ++j) {
    ta[j] = a[j];
    tb[j] = b[j];
  }
#pragma unroll 1
  for (uint32_t i = len - 1; i-- > 1;) {     // i = len - 2 ... 1
    seq_pairmul<G, K, false, true, true>(a, b, ma, mb, n, 0, sel0, qs, ts);
    load_row(ma, mb, row + (size_t)(i - 1) * (size_t)LQ);
    seq_pairmul<G, K, false, true, true>(ta, tb, a, b, n, 0, sel0, qs, ts);
  }
  // (the branches below are on launch arguments: the same way for every chain of the launch)
  if (A.out_acc) {
    seq_pairmul<G, K, false, true, true>(a, b, ma, mb, n, 0, sel0, qs, ts);
    if (live) {
      uint32_t* out = A.out_acc + ch * (size_t)LQ;
      store_pair_row<K>(out, a, x);
      store_pair_row<K>(out + L2, b, x);
    }
  }
  if (n_mul) {
    const uint32_t* mrow = A.mul + ch * (size_t)n_mul * (size_t)LQ;
    load_row(ma, mb, mrow);                  // (travels under the squarings)
#pragma unroll 1
    for (uint32_t i = 0; i < n_sqr; ++i) seq_pairmul<G, K, true, true, true>(ta, tb, ta, tb, n, 0, sel0, qs, ts);
#pragma unroll 1
    for (uint32_t k = 0; k < n_mul; ++k) {
      seq_pairmul<G, K, false, true, true>(ta, tb, ma, mb, n, 0, sel0, qs, ts);
      load_row(ma, mb, mrow + (size_t)(k + 1 < n_mul ? k + 1 : k) * (size_t)LQ);
    }
  }
  if (live) {
    uint32_t* out = A.out_tot + ch * (size_t)LQ;
    store_pair_row<K>(out, ta, x);
    store_pair_row<K>(out + L2, tb, x);
  }
}

}  // namespace pgpu

#endif  // PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_BUCKET_HPP_
