// The bit slicing behind ipcl::ext::unpackSlots (include/ipcl/ext/slots.hpp) on its own: a stand-alone program over limb
// arrays, no library, no GPU.  Every slot of every pattern is cut out of a packed limb array and compared with the value
// that went in: slot widths whose boundaries fall inside and across 64-bit words, all-ones and all-zero slots, arrays
// that end before the last slot (bits beyond the array read as zero), and the checks for bits beyond the last slot and
// for a span that overflows.  The arrays are heap blocks of exactly the stated length, so that a read past either end
// shows under -fsanitize=address,undefined.  Run by tests/test_pack_slots.py.
#include <cstdio>
#include <cstdint>
#include <random>
#include <vector>

#include "ipcl/ext/slots.hpp"

namespace sl = ipcl::ext::detail;

static long g_checks = 0, g_failed = 0;
#define CHECK(c)                                                                      \
  do {                                                                                \
    ++g_checks;                                                                       \
    if (!(c)) { ++g_failed; std::printf("  FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); } \
  } while (0)

// bit i of a little-endian limb array, zero beyond it
static int bit_of(const std::vector<uint64_t>& v, size_t i) { return i / 64 < v.size() ? (int)((v[i / 64] >> (i % 64)) & 1) : 0; }

// the packed array of `slots` values of b bits each (value t as its own limb array), built bit by bit
static std::vector<uint64_t> pack_bits(const std::vector<std::vector<uint64_t>>& vals, size_t b) {
  std::vector<uint64_t> out((vals.size() * b + 63) / 64, 0);
  for (size_t t = 0; t < vals.size(); ++t)
    for (size_t i = 0; i < b; ++i)
      if (bit_of(vals[t], i)) out[(t * b + i) / 64] |= (uint64_t)1 << ((t * b + i) % 64);
  return out;
}

static void check_pattern(const std::vector<std::vector<uint64_t>>& vals, size_t b) {
  std::vector<uint64_t> packed = pack_bits(vals, b);
  while (!packed.empty() && packed.back() == 0) packed.pop_back();          // as a BigNumber holds it: no leading zero limbs
  size_t span = 0;
  CHECK(sl::slots_span(vals.size(), b, &span) && span == vals.size() * b);
  CHECK(sl::slots_fit(packed.data(), packed.size(), span));
  std::vector<uint64_t> slot(sl::slot_limbs(b));
  CHECK(slot.size() == (b + 63) / 64);
  for (size_t t = 0; t < vals.size(); ++t) {
    for (auto& w : slot) w = ~(uint64_t)0;                                    // every limb is written
    sl::slice_slot(packed.data(), packed.size(), t * b, b, slot.data());
    bool same = true;
    for (size_t i = 0; i < 64 * slot.size(); ++i) same = same && bit_of(slot, i) == (i < b ? bit_of(vals[t], i) : 0);
    CHECK(same);
  }
}

int main() {
  std::mt19937_64 rng(7);
  for (size_t b : {(size_t)1, (size_t)7, (size_t)32, (size_t)64, (size_t)83, (size_t)63, (size_t)65, (size_t)128, (size_t)200}) {
    const size_t nl = (b + 63) / 64;
    std::vector<uint64_t> ones(nl, ~(uint64_t)0), zero(nl, 0), one(nl, 0), top(nl, 0);
    if (b % 64) ones[nl - 1] = (~(uint64_t)0) >> (64 - b % 64);
    one[0] = 1;
    top[(b - 1) / 64] = (uint64_t)1 << ((b - 1) % 64);
    for (size_t slots : {(size_t)1, (size_t)2, (size_t)3, (size_t)24, (size_t)(2047 / b), (size_t)(3071 / b)}) {
      if (slots == 0) continue;
      using V = std::vector<std::vector<uint64_t>>;
      check_pattern(V(slots, ones), b);
      check_pattern(V(slots, zero), b);
      check_pattern(V(slots, one), b);
      check_pattern(V(slots, top), b);
      V alt(slots), tla(slots), rnd(slots);
      for (size_t t = 0; t < slots; ++t) {
        alt[t] = t % 2 ? ones : zero;
        tla[t] = t % 2 ? zero : ones;
        rnd[t].resize(nl);
        for (auto& w : rnd[t]) w = rng();
        if (b % 64) rnd[t][nl - 1] &= (~(uint64_t)0) >> (64 - b % 64);
      }
      check_pattern(alt, b);
      check_pattern(tla, b);
      check_pattern(rnd, b);
      // a bit beyond the last slot does not fit; the bit below it does
      std::vector<uint64_t> over((slots * b) / 64 + 1, 0);
      over[(slots * b) / 64] = (uint64_t)1 << ((slots * b) % 64);
      CHECK(!sl::slots_fit(over.data(), over.size(), slots * b));
      CHECK(sl::slots_fit(over.data(), over.size(), slots * b + 1));
      std::vector<uint64_t> under((slots * b + 63) / 64, 0);
      under[(slots * b - 1) / 64] = (uint64_t)1 << ((slots * b - 1) % 64);
      CHECK(sl::slots_fit(under.data(), under.size(), slots * b));
      CHECK(!sl::slots_fit(under.data(), under.size(), slots * b - 1));
    }
  }
  // an empty array (the value 0) and a null pointer with no limbs
  uint64_t out[2] = {~(uint64_t)0, ~(uint64_t)0};
  sl::slice_slot(nullptr, 0, 1000, 83, out);
  CHECK(out[0] == 0 && out[1] == 0);
  CHECK(sl::slots_fit(nullptr, 0, 0) && sl::slots_fit(nullptr, 0, 5));
  // the span: zero arguments and products beyond std::size_t
  size_t span = 0;
  CHECK(!sl::slots_span(0, 8, &span) && !sl::slots_span(8, 0, &span));
  CHECK(!sl::slots_span((size_t)1 << 62, 4, &span) && !sl::slots_span(((size_t)1 << 63) + 1, 2, &span));
  CHECK(sl::slots_span(~(size_t)0, 1, &span) && span == ~(size_t)0);
  CHECK(sl::slots_span(32, 64, &span) && span == 2048);
  std::printf("%ld checks, %ld failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
