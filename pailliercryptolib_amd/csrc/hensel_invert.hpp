// pailliercryptolib_amd -- the walk back of the batched inversion on resident ciphertexts (pgpu_batch_ct_negate / _sub):
//     out[i] = x[i]^-1  mod n^2          (with mul: out[i] = mul[i] * x[i]^-1)
// by simultaneous inversion (Montgomery's trick).  The batch is cut into chains of at most `chunk` consecutive rows
// (policy.cpp: invert_plan).  The forward pass -- a one-level segscan_kernel launch -- stores the running products
// P_t = x_0 * ... * x_t of every chain; the chain totals are inverted by the same procedure, level by level, down to one
// chain whose total the host inverts; and this kernel walks every chain from its end: with U = the inverse of the chain's
// total, for t = len - 1 down to 1
//     out[t] = P[t-1] * U  ( == x_t^-1 ),     U = U * x_t  ( == P[t-1]^-1 ),       and out[0] = U.
// Two products per entry and none for the first; with the forward pass 3 (count - 1) products for a whole batch, whatever
// the chunk.  The schedule is restated in plain integers in tests/test_invert_model.py.
//
// The arithmetic is seq_pairmul of hensel_seq.hpp, lazily reduced, as in segscan_kernel: the rows stored here and there are
// valid operands on both sides of the next product.  The rows are addressed by arithmetic on the descriptors alone: no
// index list, nothing that depends on a value.
#ifndef PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_INVERT_HPP_
#define PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_INVERT_HPP_

#include "hensel_seq.hpp"

namespace pgpu {

// One wavefront = 64/G chains.  The trip count is the most steps (len - 1) any chain of the wavefront has; a group past
// its own end multiplies by the row of one -- which leaves U what it is -- and stores nothing, so that every group arrives
// at the last store with the inverse of its first entry.
// FUSED: the launch multiplies mul[t] in (A.mul != null) -- an instantiation of its own, so that the plain walk keeps the
// live set of segscan_kernel (U, P, X and the modulus: 7K registers) and only the fused one carries a fourth row.
template <int G, int K, bool FUSED>
__global__ __launch_bounds__(kWGThreads, 2) void invert_walk_kernel(InvertArgs A) {
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
  const SegscanChunk c = A.chunks[ci];
  const uint32_t len = c.len;
  // the most steps of any chain of the wavefront, in a scalar register: the loop below is the same for every group
  uint32_t longest = len - 1;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) longest = max(longest, (uint32_t)__shfl_xor((int)longest, d, kWave));
  longest = (uint32_t)__builtin_amdgcn_readfirstlane((int)longest);
  uint32_t n[K], a[K], b[K], pa[K], pb[K], xa[K], xb[K];
#pragma unroll
  for (int j = 0; j < K; ++j) n[j] = A.ctx.nhat[x * K + j];
  // step i of a chain handles its entry t = len - 1 - i, as long as that is at least 1.  No load hangs on a condition:
  // past the end the row is the row of one -- a select between two addresses, not a branch around a load
  auto live_step = [&](uint32_t i) -> bool { return i + 1 < len; };
  auto row_at = [&](const uint32_t* base, size_t t) -> const uint32_t* { return base + ((size_t)c.begin + t) * (size_t)LQ; };
  auto p_row = [&](uint32_t i) -> const uint32_t* { return live_step(i) ? row_at(A.p, len - 2 - i) : A.ctx.one; };
  auto x_row = [&](uint32_t i) -> const uint32_t* { return live_step(i) ? row_at(A.x, len - 1 - i) : A.ctx.one; };
  auto m_row = [&](uint32_t i) -> const uint32_t* { return live_step(i) ? row_at(A.mul, len - 1 - i) : A.ctx.one; };
  auto load_row = [&](uint32_t (&da)[K], uint32_t (&db)[K], const uint32_t* row) {
    load_pair_row<K>(da, row, x);
    load_pair_row<K>(db, row + L2, x);
  };
  auto store_row = [&](size_t t, const uint32_t (&sa)[K], const uint32_t (&sb)[K]) {
    uint32_t* o = A.out + ((size_t)c.begin + t) * (size_t)LQ;
    store_pair_row<K>(o, sa, x);
    store_pair_row<K>(o + L2, sb, x);
  };
  // U starts as the inverse of the chain's total.  (pa, pb) holds the running product about to be multiplied by U, (xa,
  // xb) the entry about to be multiplied into U: a row's load travels while the product before its use runs
  load_row(a, b, A.u + (size_t)c.carry * (size_t)LQ);
  load_row(pa, pb, p_row(0));
  load_row(xa, xb, x_row(0));
#pragma unroll 1
  for (uint32_t i = 0; i < longest; ++i) {
    // (no branch on a length around a product that exchanges data across the group; the store is per lane and may have one)
    if constexpr (FUSED) {
      uint32_t ma[K], mb[K];
      load_row(ma, mb, m_row(i));
      seq_pairmul<G, K, false, true, true>(pa, pb, a, b, n, 0, sel0, qs, ts);
      seq_pairmul<G, K, false, true, true>(pa, pb, ma, mb, n, 0, sel0, qs, ts);
    } else {
      seq_pairmul<G, K, false, true, true>(pa, pb, a, b, n, 0, sel0, qs, ts);
    }
    if (live_step(i) && live) store_row(len - 1 - i, pa, pb);
    // P[t-2] is read here, after the store of row t and before any store of row t - 1: p may be the memory of out
    load_row(pa, pb, p_row(i + 1));
    seq_pairmul<G, K, false, true, true>(a, b, xa, xb, n, 0, sel0, qs, ts);
    load_row(xa, xb, x_row(i + 1));
  }
  if constexpr (FUSED) {
    load_row(pa, pb, A.mul + (size_t)c.begin * (size_t)LQ);
    seq_pairmul<G, K, false, true, true>(a, b, pa, pb, n, 0, sel0, qs, ts);
  }
  if (live) store_row(0, a, b);
}

}  // namespace pgpu

#endif  // PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_INVERT_HPP_
