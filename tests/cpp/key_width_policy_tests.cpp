// CPU sweep of the rule "which pair form does an n of b bits get" (pailliercryptolib_amd/csrc/policy.cpp:
// pair_form_for_bits / pub_forms_for_bits) over EVERY width b = 16 .. 4200: the form the key builder picks (the back of the
// list capi_keys.inc: build_hensel_pub builds, taken as capi.cpp: pair_form takes it), the form the four plan calls report
// (matvec_geometry for matvec / segment_sum / segment_scan, pack_geometry for pack) and the compiled-kernel lists of
// launch.hpp must agree with each other and with the class table below.  The table is written out as class edges -- the
// numbers in the comments of launch.hpp and policy.hpp (29 G K >= bits + 29 + 8) -- and not computed by the functions under
// test.  Pure host logic: built with g++ from policy.cpp alone, no device, no HIP call.  The reference accepts any key
// length that is a multiple of 4 (ipcl/keygen.cpp:101), so none of these widths is exotic.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "launch.hpp"
#include "policy.hpp"

namespace pol = pgpu::policy;

struct Class { int lo, hi, G, K; };
// bits of n -> pair form; widths outside every class have no pair rows
static const Class kTable[] = {
    {1, 1065, 2, 19},       // 38 limbs per half: 29 * 38 = 1102 = 1065 + 37
    {1066, 2051, 4, 18},    // 72: 2088 = 2051 + 37 (1066 .. 1123 included: DESIGN.md, "Key widths off the standard classes")
    {2052, 3211, 8, 14},    // 112: 3248 = 3211 + 37
#if PGPU_WITH_4096
    {3212, 4139, 8, 18},    // 144: 4176 = 4139 + 37
#endif
};

// failures are collected per check as ranges of b, so that a broken class edge prints one line, not fifty
static std::map<std::string, std::vector<std::pair<int, int>>> g_fail;
static int g_checks = 0;
static void check(bool ok, const char* what, int b) {
  ++g_checks;
  if (ok) return;
  auto& v = g_fail[what];
  if (!v.empty() && v.back().second == b - 1) v.back().second = b;
  else v.push_back({b, b});
}

int main() {
  unsetenv("PGPU_PACK_WIDE");
  for (int b = 16; b <= 4200; ++b) {
    int EG = 0, EK = 0;   // expected
    for (const Class& c : kTable)
      if (b >= c.lo && b <= c.hi) { EG = c.G; EK = c.K; }
    const bool expect = EG != 0;
    // ---- the one rule ----
    int G = 0, K = 0;
    check(pol::pair_form_for_bits(b, &G, &K) == expect && (!expect || (G == EG && K == EK)), "pair_form_for_bits != class table", b);
    // ---- the key builder: the list's back() is the pair form iff it has the element-wise kernels (capi.cpp: pair_form) ----
    std::vector<std::pair<int, int>> forms;
    pol::pub_forms_for_bits(b, &forms);
    const bool built = !forms.empty() && pgpu::pair_ops_has(forms.back().first, forms.back().second);
    check(built == expect && (!expect || (forms.back().first == EG && forms.back().second == EK)),
          "key builder's pair form != class table", b);
    for (const auto& f : forms) {
      check(pgpu::hensel_modexp_has(f.first, f.second) || pgpu::hensel_fb_has(f.first, f.second), "key builder lists a form no kernel reads", b);
      check(29 * f.first * f.second >= b + 29 + 8, "key builder lists a form with R < 2^8 P", b);
    }
    for (size_t i = 0; i + 1 < forms.size(); ++i)
      for (size_t j = i + 1; j < forms.size(); ++j) check(forms[i] != forms[j], "key builder lists a form twice", b);
    // ---- the plan calls ----
    const bool agg = expect && pgpu::matvec_has(EG, EK);      // (the (8,18) rows of 4096-bit builds have no aggregation kernels)
    G = K = 0;
    check(pol::matvec_geometry(b, &G, &K) == agg && (!agg || (G == EG && K == EK)), "matvec_geometry != class table", b);
    G = K = 0;
    check(pol::pack_geometry(b, (size_t)1 << 20, &G, &K) == agg && (!agg || (G == EG && K == EK)), "pack_geometry (base form) != class table", b);
    const bool wide = agg && EG == 4 && EK == 18;              // (8,9) beside (4,18): launch.hpp
    G = K = 0;
    check(pol::pack_geometry(b, 1, &G, &K) == agg && (!agg || (wide ? (G == 8 && K == 9) : (G == EG && K == EK))),
          "pack_geometry (small launch) != class table", b);
    if (wide) {
      bool listed = false;
      for (const auto& f : forms) listed |= f.first == 8 && f.second == 9;
      check(listed, "plan reports the (8,9) wide form, key builder does not build it", b);
      check(forms.size() >= 2 && forms[forms.size() - 2] == std::make_pair(8, 9), "the wide form is not next to the pair form", b);
    }
    // ---- the compiled-kernel lists ----
    if (expect) {
      check(pgpu::pair_ops_has(EG, EK) && pgpu::hensel_fb_has(EG, EK) && pgpu::hensel_modexp_has(EG, EK), "pair form without element-wise / encrypt / modexp kernels", b);
      check(29 * EG * EK - (b + 29) >= 8, "class table: R < 2^8 P", b);
    }
    if (agg) {
      check(pgpu::hensel_modexp_seq_has(EG, EK) && pgpu::pair_mul_seq_has(EG, EK) && pgpu::hensel_fb_encrypt_seq_has(EG, EK),
            "pair form without sequential-halves kernels", b);
      check(pgpu::hensel_modexp_wave_has(EG * EK), "pair form without the one-wavefront kernels", b);
    }
    if (wide)
      check(pgpu::pair_ops_alt_has(8, 9) && pgpu::segsum_wide_has(8, 9) && pgpu::pack_wide_has(8, 9) &&
                pgpu::hensel_fb_encrypt_has(8, 9) && pgpu::hensel_modexp_has(8, 9), "wide form without its kernels", b);
  }
  // the edges once more by name (what the GPU tests run: tests/golden/key_widths.json)
  int G = 0, K = 0;
  check(pol::pair_form_for_bits(1065, &G, &K) && G == 2 && K == 19, "1065", 1065);
  check(pol::pair_form_for_bits(1088, &G, &K) && G == 4 && K == 18, "1088", 1088);
  check(pol::pair_form_for_bits(2051, &G, &K) && G == 4 && K == 18, "2051", 2051);
  check(pol::pair_form_for_bits(2052, &G, &K) && G == 8 && K == 14, "2052", 2052);
  check(pol::pair_form_for_bits(3211, &G, &K) && G == 8 && K == 14, "3211", 3211);
  check(pol::pair_form_for_bits(3212, &G, &K) == (PGPU_WITH_4096 != 0), "3212", 3212);
  check(!pol::pair_form_for_bits(0, &G, &K) && !pol::pair_form_for_bits(-5, &G, &K), "no width", 0);
  int failed = 0;
  for (const auto& kv : g_fail)
    for (const auto& r : kv.second) {
      std::printf("FAIL %s: b = %d .. %d\n", kv.first.c_str(), r.first, r.second);
      failed += r.second - r.first + 1;
    }
  std::printf("%d checks, %d failed\n", g_checks, failed);
  return failed ? 1 : 0;
}
