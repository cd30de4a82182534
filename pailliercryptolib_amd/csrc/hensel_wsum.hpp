// pailliercryptolib_amd -- the encrypted weighted sum of K resident ciphertext batches (pgpu_batch_ct_weighted_sum):
//     out[i] = prod_k X_k[i]^(a_k)  mod n^2          i.e.  Dec(out[i]) = sum_k a_k * Dec(X_k[i])  mod n
// K batches of one count -- K clients' encrypted vectors -- and one plaintext weight per BATCH: a federated average, or
// the plain sum when every a_k is 1.  The weights are the same for every element of the launch, so the host turns them
// into ONE bit-serial schedule (policy.cpp: wsum_plan): from the highest set bit of the weights down to bit 0 one SQR step
// per bit, then one MUL step for every term whose weight has that bit set; zero bits cost nothing for the whole launch,
// there is no window table and no per-element workspace, and the squarings are shared by all K terms.  The terms are cut
// into slices (blockIdx.y) that run their own squarings side by side where the elements alone leave SIMDs empty; the
// partial rows are folded by this same kernel with an all-MUL step list over the partial regions.  The schedule is
// restated in plain integers in tests/test_wsum_model.py.
//
// The step list is uniform for the launch: every step is read through a uniform (scalar) load and branched on
// wave-uniformly -- all lanes of every wavefront take the same path.  A branch around a seq_pairmul, which exchanges data
// across the lanes of a group, is therefore legal HERE; it is not in the kernels whose digits or lengths differ per group
// (hensel_segsum.hpp, hensel_spmv.hpp, hensel_matvec.hpp), which select operands instead.
//
// The arithmetic is seq_pairmul of hensel_seq.hpp, lazily reduced: nothing is reduced between the steps, and pair rows
// are multiplied as they lie in memory.  The rows are addressed by the element number and by the caller's PLAINTEXT
// weights (through the schedule) alone; the host refuses the call under the masked policy all the same.
#ifndef PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_WSUM_HPP_
#define PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_WSUM_HPP_

#include "hensel_seq.hpp"

namespace pgpu {

// One wavefront = 64/G elements of one slice.  (ma, mb) holds the operand of the next MUL step; at a MUL step the operand
// of the MUL after it (WsumStep::next, stored by the host) is loaded into (na, nb) before the product starts, so a row's
// load travels under the product before it and under every squaring in between.
template <int G, int K>
__global__ __launch_bounds__(kWGThreads, 2) void wsum_kernel(WsumArgs A) {
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
  size_t i = ((size_t)blockIdx.x * kWavesPerWG + wv) * IPW + grp;
  const bool live = i < A.count;
  if (!live) i = A.count - 1;   // (idle groups of the last wavefront walk the last element and do not store)
  // the plan image is written by the host before the launch and by nobody during it: read through the constant address
  // space, its loads at uniform addresses are scalar loads whatever the product blocks in between clobber
  typedef const __attribute__((address_space(4))) WsumSlice* SlicePtr;
  typedef const __attribute__((address_space(4))) WsumStep* StepPtr;
  typedef const uint32_t* const __attribute__((address_space(4)))* RowsPtr;
  const SlicePtr sl = (SlicePtr)A.slices + blockIdx.y;
  const StepPtr steps = (StepPtr)A.steps + sl->step_begin;
  const RowsPtr rows = (RowsPtr)A.rows;
  const uint32_t n_steps = sl->n_steps;
  const size_t off = i * (size_t)LQ;
  uint32_t n[K], a[K], b[K], ma[K], mb[K];
#pragma unroll
  for (int j = 0; j < K; ++j) n[j] = A.ctx.nhat[x * K + j];
  // the row of a term for this element.  The term is uniform: a scalar select between two addresses, both valid, not a
  // branch around a load (kWsumNone: the row of one, read where the schedule has nothing left to stage)
  auto row_of = [&](uint32_t term) -> const uint32_t* {
    const uint32_t* base = rows[term == kWsumNone ? 0u : term];
    return term == kWsumNone ? A.ctx.one : base + off;
  };
  auto load_row = [&](uint32_t (&da)[K], uint32_t (&db)[K], const uint32_t* row) {
    load_pair_row<K>(da, row, x);
    load_pair_row<K>(db, row + L2, x);
  };
  load_row(a, b, row_of(sl->first));
  load_row(ma, mb, row_of(sl->first_mul));
#pragma unroll 1
  for (uint32_t t = 0; t < n_steps; ++t) {
    const uint32_t op = steps[t].op;
    if (op == kWsumSqr) {
      seq_pairmul<G, K, true, true, true>(a, b, a, b, n, 0, sel0, qs, ts);
    } else {
      uint32_t na[K], nb[K];
      load_row(na, nb, row_of(steps[t].next));
      seq_pairmul<G, K, false, true, true>(a, b, ma, mb, n, 0, sel0, qs, ts);
#pragma unroll
      for (int j = 0; j < K; ++j) {
        ma[j] = na[j];
        mb[j] = nb[j];
      }
    }
  }
  if (live) {
    uint32_t* out = sl->dst + off;
    store_pair_row<K>(out, a, x);
    store_pair_row<K>(out + L2, b, x);
  }
}

}  // namespace pgpu

#endif  // PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_WSUM_HPP_
