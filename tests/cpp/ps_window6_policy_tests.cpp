// CPU unit test of the window rule of the one-lane CRT decrypt (pailliercryptolib_amd/csrc/policy.cpp: pick_decrypt_window
// with one_lane = true): the width of the least count of pair squarings and pair products, weighted by the instructions of
// the two loops, on the half-squared table.  Pure host logic -- built with g++ from policy.cpp alone, no device, no HIP call.
// The exponentiations it steers are the two of PrivateKey::decryptCRT (ipcl/pri_key.cpp:114-146).
#include <cstdio>

#include "policy.hpp"

namespace pol = pgpu::policy;
static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      ++g_failed;                                                          \
      std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);          \
    }                                                                      \
  } while (0)

// the count the rule minimises, written out again: (squarings, products) of one exponentiation
static long weighted(int bits, int w) {
  const long nwin = (bits + w - 1) / w, build = (1L << (w - 1)) - 1;
  return ((nwin - 1) * w + build) * 5260 + ((nwin - 1) + build) * 7278;
}

int main() {
  const size_t headline = (size_t)2 * 8192 * 2 * 36 * 4;      // one table entry of every exponentiation: 8192 ciphertexts, K = 36
  // 1024-bit exponents (2048-bit keys): 1051 squarings + 201 products at w = 6 against 1035 + 219 at w = 5
  CHECK(weighted(1024, 6) == 1051L * 5260 + 201L * 7278 && weighted(1024, 5) == 1035L * 5260 + 219L * 7278);
  CHECK(weighted(1024, 6) < weighted(1024, 5));
  CHECK(pol::pick_decrypt_window(1024, headline, true) == 6 && pol::pick_decrypt_window(1024, 0, true) == 6);
  // the other forms keep their rule
  CHECK(pol::pick_decrypt_window(1024, headline, false) == 5 && pol::pick_decrypt_window(1024) == 5);
  // 512-bit exponents stay at 5, 1536- and 2048-bit ones at 6 (as before)
  CHECK(pol::pick_decrypt_window(512, 0, true) == 5 && pol::pick_decrypt_window(1536, 0, true) == 6 && pol::pick_decrypt_window(2048, 0, true) == 6);
  // every width is the minimum of the weighted count over 1..6
  for (int bits : {1, 7, 33, 100, 256, 512, 768, 1013, 1024, 1040, 1280, 1536, 2048}) {
    const int w = pol::pick_decrypt_window(bits, 0, true);
    CHECK(w >= 1 && w <= 6);
    for (int v = 1; v <= 6; ++v) CHECK(weighted(bits, w) <= weighted(bits, v));
  }
  // the table cap of 4 GiB is on the sixth bit: 2^6 entries of more than 64 MiB each fall back to 5
  CHECK(pol::pick_decrypt_window(1024, ((size_t)4 << 30) / 64, true) == 6 && pol::pick_decrypt_window(1024, ((size_t)4 << 30) / 64 + 1, true) == 5);
  CHECK(pol::pick_decrypt_window(1536, (size_t)2 * (1 << 20) * 448, true) == 5);
  // a forced width holds for every form, and 0 gives the rules back
  CHECK(pol::set_fixed_window(5) == 0);
  CHECK(pol::pick_decrypt_window(1024, headline, true) == 5 && pol::pick_window(33) == 5);
  CHECK(pol::set_fixed_window(6) == 5);
  CHECK(pol::pick_decrypt_window(1024, headline, true) == 6 && pol::pick_decrypt_window(1024, headline, false) == 6 && pol::pick_window(1024) == 6);
  CHECK(pol::set_fixed_window(9) == 6 && pol::set_fixed_window(-3) == 6 && pol::set_fixed_window(0) == 0);
  CHECK(pol::pick_decrypt_window(1024, headline, true) == 6 && pol::pick_window(1024) == 5 && pol::masked_decrypt_window() == 3);
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
