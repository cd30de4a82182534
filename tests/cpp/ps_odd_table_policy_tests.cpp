// CPU unit test of the window rule of the one-lane CRT decrypt beside the ODD-POWER window table
// (pailliercryptolib_amd/csrc/policy.cpp: ps_one_lane_ops, pick_decrypt_window with one_lane = true, ps_odd_table): the counts
// of the two table forms, and that the widths the rule picks are the ones the odd form's own counts pick for the exponent
// classes the one-lane kernels serve.  Pure host logic -- built with g++ from policy.cpp alone, no device, no HIP call.
// The exponentiations it steers are the two of PrivateKey::decryptCRT (ipcl/pri_key.cpp:114-146).
#include <cstdio>

#include "launch.hpp"
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

static long sq(int bits, int w, bool odd) {
  long s, m;
  pol::ps_one_lane_ops(bits, w, odd, &s, &m);
  return s;
}
static long mu(int bits, int w, bool odd) {
  long s, m;
  pol::ps_one_lane_ops(bits, w, odd, &s, &m);
  return m;
}
// instructions of one exponentiation: the loops of hensel_decrypt_psb_kernel<36,29,1>
static long weighted(int bits, int w, bool odd) { return sq(bits, w, odd) * 5145 + mu(bits, w, odd) * 7278; }

int main(int argc, char** argv) {
  const bool expect_odd = !(argc > 1 && argv[1][0] == '0');
  CHECK((pol::ps_odd_table() != 0) == expect_odd);             // PGPU_PS_ODD_TABLE: default 1, 0 switches it off
  const size_t headline = (size_t)2 * 8192 * 2 * 36 * 4;       // one table entry of every exponentiation: 8192 ciphertexts, K = 36
  // the counts: half-squared 1051 + 201, odd powers 1025 + 202 at w = 6 -- 26 squarings fewer, one product more
  CHECK(sq(1024, 6, false) == 1051 && mu(1024, 6, false) == 201 && sq(1024, 5, false) == 1035 && mu(1024, 5, false) == 219);
  CHECK(sq(1024, 6, true) == 1025 && mu(1024, 6, true) == 202);
  CHECK(weighted(1024, 6, true) - weighted(1024, 6, false) == -26L * 5145 + 7278);
  CHECK(mu(1024, 5, true) == 220 && mu(1024, 7, true) == 210);
  // the squarings of the odd form do not depend on the width (one for base^2, one per exponent bit), nor on the exponent
  for (int bits : {512, 1013, 1024, 1040, 1536})
    for (int w = 2; w <= 7; ++w) CHECK(sq(bits, w, true) == bits + 1);
  CHECK(sq(1024, 1, true) == 1024 && mu(1024, 1, true) == 1024);       // (w = 1: no chain, no base^2)
  // 1024 bits: 6 is the best width by the odd counts too, also against 7
  for (int w = 1; w <= 7; ++w) CHECK(weighted(1024, 6, true) <= weighted(1024, w, true));
  CHECK(pol::pick_decrypt_window(1024, headline, true) == 6);
  // 1536 bits: 6 among 1..6; the seventh bit would save 4 products, under 0.5 % of the exponentiation
  for (int w = 1; w <= 6; ++w) CHECK(weighted(1536, 6, true) <= weighted(1536, w, true));
  CHECK(mu(1536, 6, true) - mu(1536, 7, true) == 4 && (weighted(1536, 6, true) - weighted(1536, 7, true)) * 200 < weighted(1536, 6, true));
  CHECK(pol::pick_decrypt_window(1536, 0, true) == 6);
  // 512 bits: the rule stays at 5; 6 would save ONE product, under 0.5 % of the exponentiation, for twice the table
  CHECK(mu(512, 5, true) == 118 && mu(512, 6, true) == 117);
  CHECK((weighted(512, 5, true) - weighted(512, 6, true)) * 200 < weighted(512, 5, true));
  for (int w = 1; w <= 5; ++w) CHECK(weighted(512, 5, true) <= weighted(512, w, true));
  CHECK(pol::pick_decrypt_window(512, 0, true) == 5);
  // for every exponent length of a prime the one-lane kernels take -- K = 19 limbs of 29 bits: primes of 490 .. 518 bits; K = 38
  // of 28, with K = 36 balanced of 29 beside it: 1005 .. 1032 (swept to the 1040 bits the balanced limbs hold); K = 56 of 28:
  // 1509 .. 1536 (capi_keys.inc: build_hensel picks the K with LB K >= bits + LB + 4 > LB (K - 1), and only these K are
  // instantiated) -- the width the rule picks is within 0.5 % of the odd form's best over 1..6.  (Between the classes it is
  // not: a 700-bit exponent would gain 1.1 % at w = 6.)
  const int classes[3][2] = {{490, 518}, {1005, 1040}, {1509, 1536}};
  for (const auto& c : classes)
    for (int bits = c[0]; bits <= c[1]; ++bits) {
      const int w = pol::pick_decrypt_window(bits, 0, true);
      CHECK(w == (c[0] < 600 ? 5 : 6));
      for (int v = 1; v <= 6; ++v) CHECK((weighted(bits, w, true) - weighted(bits, v, true)) * 200 < weighted(bits, w, true));
    }
  // the width does not depend on the table form, nor does the cap on the sixth bit
  const int was = pol::set_ps_odd_table(0);
  CHECK(was == (expect_odd ? 1 : 0) && pol::ps_odd_table() == 0);
  CHECK(pol::pick_decrypt_window(1024, headline, true) == 6 && pol::pick_decrypt_window(512, 0, true) == 5);
  CHECK(pol::set_ps_odd_table(7) == 0 && pol::ps_odd_table() == 1);
  CHECK(pol::pick_decrypt_window(1024, ((size_t)4 << 30) / 64, true) == 6 && pol::pick_decrypt_window(1024, ((size_t)4 << 30) / 64 + 1, true) == 5);
  pol::set_ps_odd_table(was);
  // the table: 2^(w-1) + 1 entries instead of 2^w; the headline's launch 156 MB instead of 302 MB
  CHECK(pgpu::hensel_ps_table_entries(6, true) == 33 && pgpu::hensel_ps_table_entries(6, false) == 64);
  CHECK(pgpu::hensel_ps_table_entries(1, true) == 2 && pgpu::hensel_ps_table_entries(1, false) == 2);
  CHECK(pgpu::hensel_ps_table_entries(5, true) == 17 && pgpu::hensel_ps_table_entries(3, false) == 8);
  const size_t waves = 2 * 8192 / 64;
  CHECK(waves * pgpu::hensel_ps_table_words(36, 64) * 4 == (size_t)301989888 && waves * pgpu::hensel_ps_table_words(36, 33) * 4 == (size_t)155713536);
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
