// ipcl::ext -- bit slicing of packed plaintexts (the host side of packSlots / unpackSlots, ipcl/ext/aggregate.hpp): plain
// functions over little-endian 64-bit limb arrays, header-only and free of every other header of the library, so that
// they can be exercised on their own (tests/cpp/slots_slicing_tests.cpp).
#ifndef PAILLIERCRYPTOLIB_AMD_IPCL_EXT_SLOTS_HPP_
#define PAILLIERCRYPTOLIB_AMD_IPCL_EXT_SLOTS_HPP_

#include <cstddef>
#include <cstdint>

namespace ipcl {
namespace ext {
namespace detail {

// seg_len * slot_bits as bits, false when either is zero or the product does not fit std::size_t
inline bool slots_span(std::size_t seg_len, std::size_t slot_bits, std::size_t* bits) {
  if (seg_len == 0 || slot_bits == 0 || seg_len > ~(std::size_t)0 / slot_bits) return false;
  *bits = seg_len * slot_bits;
  return true;
}

// no bit of (limbs, n_limbs) is set at position `bits` or above
inline bool slots_fit(const uint64_t* limbs, std::size_t n_limbs, std::size_t bits) {
  const std::size_t word = bits / 64, sh = bits % 64;
  for (std::size_t i = word; i < n_limbs; ++i) {
    const uint64_t v = i == word ? (sh ? limbs[i] >> sh : limbs[i]) : limbs[i];
    if (v) return false;
  }
  return true;
}

// limbs needed for one slot
inline std::size_t slot_limbs(std::size_t slot_bits) { return slot_bits / 64 + (slot_bits % 64 ? 1 : 0); }

// out[0 .. slot_limbs(slot_bits)) = bits [at, at + slot_bits) of (limbs, n_limbs); bits beyond the array read as zero.
// at + slot_bits must not overflow (slots_span of the whole row holds that).
inline void slice_slot(const uint64_t* limbs, std::size_t n_limbs, std::size_t at, std::size_t slot_bits, uint64_t* out) {
  const std::size_t n_out = slot_limbs(slot_bits), word = at / 64, sh = at % 64;
  for (std::size_t i = 0; i < n_out; ++i) {
    const std::size_t lo = word + i;
    uint64_t v = lo < n_limbs ? limbs[lo] >> sh : 0;
    if (sh && lo + 1 < n_limbs) v |= limbs[lo + 1] << (64 - sh);
    out[i] = v;
  }
  if (slot_bits % 64) out[n_out - 1] &= (~(uint64_t)0) >> (64 - slot_bits % 64);
}

}  // namespace detail
}  // namespace ext
}  // namespace ipcl
#endif  // PAILLIERCRYPTOLIB_AMD_IPCL_EXT_SLOTS_HPP_
