// pailliercryptolib_amd -- row_gather_kernel: re-indexing of resident batches (pgpu_batch_gather, the strided
// pgpu_batch_slice).  out[i] = row d.row of source d.source, rows moved as BYTES: no arithmetic, no key, no domain --
// plain words of any width, Montgomery words and pair rows alike (304 / 576 / 896 bytes for the pair rows of 1024- /
// 2048- / 3072-bit keys, 8 * words bytes otherwise; rows of 8 bytes included).
//
// A row is swept by a GROUP of neighbouring lanes in contiguous pieces of 16 bytes (row_bytes % 16 == 0) or 8 bytes: lane x
// of the group moves pieces x, x + lanes, ... -- a wave-instruction reads 64/lanes contiguous runs of lanes * piece bytes,
// never 64 lanes in 64 rows.  A group has at most 16 lanes, so a wavefront keeps at least four rows in flight, and every
// lane issues up to four loads before its first store (policy.hpp: gather_plan has the numbers; the host chooses, the
// kernel obeys).
//
// The descriptor's row of all ones is the sentinel: the row of "one" (the integer 1, R mod N, the pair row of one) is read
// instead -- a select between two addresses, both valid, not a branch around a load (hensel_wsum.hpp: row_of).  Idle
// groups of the last wavefront walk the last output and do not store.  The address stream depends on the caller's
// plaintext indices only.
#ifndef PAILLIERCRYPTOLIB_AMD_CSRC_GATHER_HPP_
#define PAILLIERCRYPTOLIB_AMD_CSRC_GATHER_HPP_

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "kargs.hpp"

namespace pgpu {

constexpr uint32_t kGatherOneRow = 0xFFFFFFFFu;   // GatherDesc::row: the row of one
constexpr int kGatherMaxLanes = 16;               // lanes per row at most: four rows in flight per wavefront at least
constexpr int kGatherUnroll = 4;                  // loads a lane issues before its first store

struct GatherDesc {   // one per output row
  uint32_t source;    // entry of the table of source bases (any valid entry beside the sentinel)
  uint32_t row;       // row of that source, or kGatherOneRow
};
static_assert(sizeof(GatherDesc) == 8, "one 8-byte descriptor per output");

struct GatherArgs {
  const GatherDesc* desc;        // [n_out]
  const char* const* bases;      // [n_src] first byte of every source
  const char* one;               // one row holding "one"
  char* out;                     // [n_out] rows, dense
  size_t n_out;
  uint32_t row_bytes;            // a multiple of the piece size
  uint32_t lanes_log2;           // lanes per row = 1 << lanes_log2  (<= kGatherMaxLanes)
};

// vec_bytes: 16 or 8 (policy.hpp: gather_plan); false: no such instantiation
bool launch_row_gather(int vec_bytes, const GatherArgs& a, unsigned blocks, hipStream_t s);

#ifdef __HIPCC__
typedef uint32_t gather_piece16 __attribute__((ext_vector_type(4)));
typedef uint32_t gather_piece8 __attribute__((ext_vector_type(2)));

// V: gather_piece16 or gather_piece8
template <class V>
__global__ __launch_bounds__(kWGThreads) void row_gather_kernel(GatherArgs A) {
  static_assert(kGatherUnroll == 4, "the loop body below is written out for four pieces");
  const uint32_t lanes = 1u << A.lanes_log2, rpw = (uint32_t)kWave >> A.lanes_log2;
  const uint32_t lane = threadIdx.x % kWave, wv = threadIdx.x / kWave;
  const uint32_t grp = lane >> A.lanes_log2, x = lane & (lanes - 1);
  size_t i = ((size_t)blockIdx.x * kWavesPerWG + wv) * rpw + grp;
  const bool live = i < A.n_out;
  if (!live) i = A.n_out - 1;   // (idle groups of the last wavefront walk the last output and do not store)
  const uint64_t d = *(const uint64_t*)(A.desc + i);   // {source, row} in one load
  const uint32_t row = (uint32_t)(d >> 32);
  const bool is_one = row == kGatherOneRow;
  // the sentinel: a select between two addresses, both valid, not a branch around a load.  (The empty asm makes the
  // table entry a value the compiler has to have: it does not sink the load into a branch on is_one.)
  uintptr_t base = (uintptr_t)A.bases[is_one ? 0u : (uint32_t)d];
  asm volatile("" : "+v"(base));
  const uintptr_t from = is_one ? (uintptr_t)A.one : base + (uintptr_t)row * A.row_bytes;
  // (global address space, said so: the table's entries are generic pointers to the compiler)
  const __attribute__((address_space(1))) V* src = (const __attribute__((address_space(1))) V*)from;
  __attribute__((address_space(1))) V* dst = (__attribute__((address_space(1))) V*)(uintptr_t)(A.out + i * (size_t)A.row_bytes);
  const uint32_t pieces = A.row_bytes / (uint32_t)sizeof(V), last = pieces - 1;
#pragma unroll 1
  for (uint32_t p = x; p < pieces; p += kGatherUnroll * lanes) {
    const uint32_t q1 = p + lanes, q2 = p + 2 * lanes, q3 = p + 3 * lanes;
    // four loads in flight before the first store; past the row's end a lane reads the last piece again and stores nothing
    V v0 = src[p], v1 = src[q1 < pieces ? q1 : last], v2 = src[q2 < pieces ? q2 : last], v3 = src[q3 < pieces ? q3 : last];
    asm volatile("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3));
    if (live) {
      dst[p] = v0;
      if (q1 < pieces) dst[q1] = v1;
      if (q2 < pieces) dst[q2] = v2;
      if (q3 < pieces) dst[q3] = v3;
    }
  }
}
#endif  // __HIPCC__

}  // namespace pgpu

#endif  // PAILLIERCRYPTOLIB_AMD_CSRC_GATHER_HPP_
