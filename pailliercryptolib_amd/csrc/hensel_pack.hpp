// pailliercryptolib_amd -- the encrypted slot packing of resident ciphertexts (pgpu_batch_ct_pack):
//     out[r] = prod_t X[r][t]^(2^(b t))  mod n^2      i.e.  Dec(out[r]) = sum_t Dec(X[r][t]) * 2^(b t)  mod n
// x is read as [rows][seg_len]; b = slot_bits; slot 0 is the least significant.  One ciphertext then carries seg_len
// values of b bits each: the key holder decrypts one row where it decrypted seg_len (FATE's SecureBoost+ calls it
// "cipher compressing").  By Horner a packed row is one chain: start as the last entry, then for t = seg_len - 2 ... 0
// square b times and multiply by entry t -- the two calls of seq_pairmul that hensel_modexp_seq_kernel alternates, with
// the entries of the row in the place of its window table.  The schedule is restated in plain integers in
// tests/test_pack_model.py.
//
// The arithmetic is seq_pairmul of hensel_seq.hpp, lazily reduced: nothing is reduced between the steps, and the row a
// chain stores comes out of a product (or is the input row when seg_len == 1), so it is a valid operand on both sides of
// the next product anywhere.  The rows are addressed by arithmetic on rows and seg_len alone: no descriptors, no index
// list, nothing that depends on a value; every chain of a launch has the same trip count.
#ifndef PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_PACK_HPP_
#define PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_PACK_HPP_

#include "hensel_seq.hpp"

namespace pgpu {

// One wavefront = 64/G output rows.  (ma, mb) holds the entry about to be multiplied in: its load is issued right after
// the product that consumed the entry before it and travels under the slot_bits squarings -- no third staged row.
template <int G, int K>
__global__ __launch_bounds__(kWGThreads, 2) void pack_kernel(PackArgs A) {
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
  size_t r = ((size_t)blockIdx.x * kWavesPerWG + wv) * IPW + grp;
  const bool live = r < A.rows;
  if (!live) r = A.rows - 1;   // (idle groups of the last wavefront walk a valid row and do not store)
  const uint32_t len = A.seg_len, bits = A.slot_bits;
  const uint32_t* row = A.src + r * (size_t)len * (size_t)LQ;
  uint32_t n[K], a[K], b[K], ma[K], mb[K];
#pragma unroll
  for (int j = 0; j < K; ++j) n[j] = A.ctx.nhat[x * K + j];
  auto load_entry = [&](uint32_t (&da)[K], uint32_t (&db)[K], uint32_t t) {
    const uint32_t* e = row + (size_t)t * (size_t)LQ;
    load_pair_row<K>(da, e, x);
    load_pair_row<K>(db, e + L2, x);
  };
  // no load hangs on a condition: a row of one entry reads it twice, and the last step reads entry 0 again
  load_entry(a, b, len - 1);
  load_entry(ma, mb, len > 1 ? len - 2 : 0);
#pragma unroll 1
  for (uint32_t t = len - 1; t-- > 0;) {
#pragma unroll 1
    for (uint32_t i = 0; i < bits; ++i) seq_pairmul<G, K, true, true, true>(a, b, a, b, n, 0, sel0, qs, ts);
    seq_pairmul<G, K, false, true, true>(a, b, ma, mb, n, 0, sel0, qs, ts);
    load_entry(ma, mb, t ? t - 1 : 0);
  }
  if (live) {
    uint32_t* out = A.out + r * (size_t)LQ;
    store_pair_row<K>(out, a, x);
    store_pair_row<K>(out + L2, b, x);
  }
}

}  // namespace pgpu

#endif  // PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_PACK_HPP_
