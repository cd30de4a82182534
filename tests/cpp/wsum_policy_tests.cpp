// CPU unit test of the host schedule of the encrypted weighted sum of K resident batches
// (pailliercryptolib_amd/csrc/policy.cpp: wsum_*): weights -> slices and step lists, (count, n_terms) -> S, chains -> form.
// Pure host logic -- built with g++ from policy.cpp alone, no device, no HIP call.  With the argument "plan" the binary
// reads "n_terms w_words S unit" and n_terms * w_words hexadecimal words from stdin and prints the schedule
// (tests/test_wsum_model.py walks it in integers).  In the reference such a sum is composed from CipherText::operator*
// (ipcl/ciphertext.cpp:83-106) and operator+ (ciphertext.cpp:35-72) term by term; the rule is documented in DESIGN.md
// ("Encrypted weighted sum of K resident batches").
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "policy.hpp"

namespace pol = pgpu::policy;
using pgpu::kWsumNone;
using pgpu::kWsumSqr;
using pgpu::WsumSlice;
using pgpu::WsumStep;
static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      ++g_failed;                                                          \
      std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);          \
    }                                                                      \
  } while (0)

static int print_plan() {
  size_t n_terms = 0, S = 0;
  int w_words = 0, unit = 0;
  if (std::scanf("%zu %d %zu %d", &n_terms, &w_words, &S, &unit) != 4) return 2;
  std::vector<uint64_t> w(unit ? 0 : n_terms * (size_t)w_words);
  for (auto& v : w)
    if (std::scanf("%lx", &v) != 1) return 2;
  pol::WsumPlan plan;
  if (!pol::wsum_plan(unit ? nullptr : w.data(), w_words, n_terms, S, &plan)) {
    std::printf("refused\n");
    return 0;
  }
  std::printf("plan %zu %zu %zu %zu %zu %d\n", plan.slices.size(), plan.longest, plan.squarings, plan.muls, plan.products,
              plan.all_zero ? 1 : 0);
  for (const WsumSlice& sl : plan.slices) {
    std::printf("slice %u %u %u %u %u\n", sl.term_begin, sl.term_end, sl.first, sl.first_mul, sl.n_steps);
    for (size_t t = 0; t < sl.n_steps; ++t) {
      const WsumStep& st = plan.steps[(size_t)sl.step_begin + t];
      std::printf("%u %u\n", st.op, st.next);
    }
  }
  return 0;
}

static size_t bitlen(const uint64_t* w, size_t ww) {
  for (size_t j = ww; j-- > 0;)
    if (w[j]) return 64 * j + (size_t)(64 - __builtin_clzll(w[j]));
  return 0;
}
static bool bit_of(const uint64_t* w, size_t b) { return (w[b >> 6] >> (b & 63)) & 1; }

// the schedule of a plan against the weights it was made for
static void check_plan(const std::vector<uint64_t>& w, int w_words, size_t n_terms, size_t S) {
  const bool unit = w.empty();
  const size_t ww = unit ? 1 : (size_t)w_words;
  std::vector<uint64_t> ones(n_terms, 1);
  const uint64_t* W = unit ? ones.data() : w.data();
  pol::WsumPlan plan;
  CHECK(pol::wsum_plan(unit ? nullptr : w.data(), w_words, n_terms, S, &plan));
  const size_t Sc = S < n_terms ? S : n_terms;
  // the slices partition the terms: contiguous ranges of the rule, the all-zero ones dropped
  size_t want_sq = 0, want_mul = 0, want_slices = 0, want_longest = 0, si = 0;
  std::vector<std::vector<int>> seen(n_terms, std::vector<int>(64 * ww, 0));
  for (size_t s = 0; s < Sc; ++s) {
    const size_t lo = s * n_terms / Sc, hi = (s + 1) * n_terms / Sc;
    CHECK(hi > lo);
    size_t top = 0, pops = 0;
    for (size_t k = lo; k < hi; ++k) {
      const size_t L = bitlen(W + k * ww, ww);
      top = L > top ? L : top;
      for (size_t b = 0; b < L; ++b) pops += bit_of(W + k * ww, b);
    }
    if (!pops) continue;
    ++want_slices;
    want_sq += top - 1;
    want_mul += pops - 1;
    want_longest = top - 1 + pops - 1 > want_longest ? top - 1 + pops - 1 : want_longest;
    CHECK(si < plan.slices.size());
    if (si >= plan.slices.size()) return;
    const WsumSlice& sl = plan.slices[si++];
    CHECK(sl.term_begin == lo && sl.term_end == hi);
    CHECK(sl.n_steps == top - 1 + pops - 1);
    CHECK((size_t)sl.step_begin + sl.n_steps <= plan.steps.size());
    // walk the list: the bit position falls by one at every SQR; every MUL names a term of the slice whose weight has the
    // current bit set, in term order within a bit; `next` names the MUL after it
    size_t bit = top - 1, sq = 0;
    CHECK(sl.first >= lo && sl.first < hi && bit_of(W + sl.first * ww, bit));
    if (sl.first < n_terms) ++seen[sl.first][bit];
    uint32_t expect = sl.first_mul, last_term = sl.first;
    size_t last_bit = bit;
    for (size_t t = 0; t < sl.n_steps; ++t) {
      const WsumStep& st = plan.steps[(size_t)sl.step_begin + t];
      if (st.op == kWsumSqr) {
        CHECK(bit > 0);
        --bit;
        ++sq;
        continue;
      }
      CHECK(st.op == expect);
      CHECK(st.op >= lo && st.op < hi);
      if (st.op >= n_terms) return;
      CHECK(bit_of(W + st.op * ww, bit));
      CHECK(bit < last_bit || st.op > last_term);      // term order within a bit
      ++seen[st.op][bit];
      last_term = st.op;
      last_bit = bit;
      expect = st.next;
    }
    CHECK(expect == kWsumNone);                        // nothing is staged past the last MUL
    CHECK(bit == 0 && sq == top - 1);
  }
  if (want_slices == 0) {
    CHECK(plan.all_zero && plan.slices.size() == 1 && plan.steps.empty() && plan.products == 0);
    CHECK(plan.slices[0].first == kWsumNone && plan.slices[0].first_mul == kWsumNone && plan.slices[0].n_steps == 0);
    return;
  }
  CHECK(!plan.all_zero && plan.slices.size() == want_slices && si == want_slices);
  CHECK(plan.squarings == want_sq && plan.muls == want_mul && plan.longest == want_longest);
  CHECK(plan.steps.size() == want_sq + want_mul);
  CHECK(plan.products == want_sq + want_mul + want_slices - 1);
  // every set bit of every weight appears exactly once, no clear bit at all
  for (size_t k = 0; k < n_terms; ++k)
    for (size_t b = 0; b < 64 * ww; ++b) CHECK(seen[k][b] == (bit_of(W + k * ww, b) ? 1 : 0));
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "plan")) return print_plan();
  unsetenv("PGPU_WSUM_SLICES");
  unsetenv("PGPU_WSUM_WIDE");
  // ---- schedules of ragged weights ----
  for (size_t n_terms : {1u, 2u, 3u, 5u, 17u, 64u})
    for (int w_words : {1, 2, 3})
      for (size_t S : {1u, 2u, 3u, 4u, 17u, 100u}) {
        std::vector<uint64_t> w(n_terms * (size_t)w_words, 0);
        for (size_t k = 0; k < n_terms; ++k) {
          const int kind = (int)(rnd() % 7);
          uint64_t* p = &w[k * (size_t)w_words];
          if (kind == 0) continue;                                      // zero
          if (kind == 1) { p[0] = 1; continue; }
          if (kind == 2) { p[w_words - 1] = 1ull << 63; continue; }     // a lone top bit
          if (kind == 3) { for (int j = 0; j < w_words; ++j) p[j] = ~0ull; continue; }   // 2^e - 1
          if (kind == 4) { p[0] = rnd() & 0xFFFFFFFFull; continue; }
          for (int j = 0; j < w_words; ++j) p[j] = rnd();
          if (kind == 6) p[w_words - 1] >>= (rnd() % 64);
        }
        check_plan(w, w_words, n_terms, S);
      }
  for (size_t n_terms : {1u, 2u, 3u, 5u, 17u})
    for (size_t S : {1u, 2u, 3u, 17u}) {
      check_plan({}, 0, n_terms, S);                                    // no weights: all ones
      check_plan(std::vector<uint64_t>(n_terms * 2, 0), 2, n_terms, S); // every weight zero
    }
  {
    // the issue's count: 16 random 32-bit weights, one slice: 31 squarings + (popcounts - 1) products
    std::vector<uint64_t> w(16);
    size_t pops = 0;
    for (auto& v : w) {
      v = (rnd() & 0xFFFFFFFFull) | 0x80000000ull;
      pops += (size_t)__builtin_popcountll(v);
    }
    pol::WsumPlan plan;
    CHECK(pol::wsum_plan(w.data(), 1, 16, 1, &plan));
    CHECK(plan.squarings == 31 && plan.muls == pops - 1 && plan.products == 31 + pops - 1 && plan.longest == plan.products);
    // the same terms in 4 slices: 4 x 31 squarings, the same products less 3 loads, 3 fold products
    CHECK(pol::wsum_plan(w.data(), 1, 16, 4, &plan));
    CHECK(plan.slices.size() == 4 && plan.squarings == 4 * 31 && plan.muls == pops - 4 && plan.products == 4 * 31 + pops - 4 + 3);
    // one term, weight 1: a copy -- no step, no product
    const uint64_t one = 1;
    CHECK(pol::wsum_plan(&one, 1, 1, 1, &plan));
    CHECK(plan.slices.size() == 1 && plan.steps.empty() && plan.products == 0 && plan.slices[0].first == 0 && !plan.all_zero);
  }
  // ---- refusals of the plan ----
  {
    pol::WsumPlan plan;
    plan.longest = 77;
    const uint64_t one = 1;
    CHECK(!pol::wsum_plan(&one, 1, 0, 1, &plan));
    CHECK(!pol::wsum_plan(&one, 0, 1, 1, &plan));
    CHECK(!pol::wsum_plan(&one, 1, 1, 0, &plan));
    CHECK(!pol::wsum_plan(nullptr, 0, pol::kWsumMaxTerms + 1, 1, &plan));
    CHECK(pol::wsum_plan(nullptr, 0, pol::kWsumMaxTerms, 1, &plan) && plan.muls == pol::kWsumMaxTerms - 1);
    // one weight with a lone bit at 2^31: 2^31 squarings -- refused from the bit lengths, before anything is written
    // (the words come zeroed from calloc and are only read)
    const size_t words = ((size_t)1 << 25) + 1;
    uint64_t* big = (uint64_t*)std::calloc(words, sizeof(uint64_t));
    CHECK(big != nullptr);
    if (big) {
      big[words - 1] = 1;
      plan = pol::WsumPlan();
      plan.longest = 77;
      CHECK(!pol::wsum_plan(big, (int)words, 1, 1, &plan));
      CHECK(plan.longest == 77 && plan.slices.empty());
      std::free(big);
    }
  }
  // ---- S: the matvec's rule ----
  for (int G : {2, 4, 8}) {
    const size_t ipw = 64 / (size_t)G;
    for (size_t count : {1u, 17u, 256u, 8192u, 16384u, 65536u, 1000000u})
      for (size_t n : {1u, 2u, 3u, 4u, 7u, 8u, 16u, 64u, 4096u}) {
        const size_t waves = (count + ipw - 1) / ipw, fill = (pol::kSimds + waves - 1) / waves;
        for (bool unit : {false, true}) {
          const size_t cap = n / (unit ? 2 : pol::kMatvecMinSliceCols) ? n / (unit ? 2 : pol::kMatvecMinSliceCols) : 1;
          const size_t want = fill < cap ? fill : cap;
          const size_t S = pol::wsum_slices(G, count, n, unit);
          CHECK(S == (want < 1 ? 1 : want));
          CHECK(S >= 1 && S <= n);
          if (!unit && S > 1) CHECK(n / S >= pol::kMatvecMinSliceCols);
          if (unit && S > 1) CHECK(n / S >= 2);
          if (S > 1) CHECK((S - 1) * waves < pol::kSimds);              // the smallest S that fills
        }
      }
  }
  CHECK(pol::wsum_slices(4, 65536, 16, false) == 1);                   // 4096 wavefronts: the elements alone fill the chip
  CHECK(pol::wsum_slices(4, 256, 16, false) == 4);                     // 16 wavefronts: the cap of 4 terms per slice binds
  CHECK(pol::wsum_slices(4, 256, 16, true) == 8);
  // ---- the forced knobs ----
  setenv("PGPU_WSUM_SLICES", "3", 1);
  CHECK(pol::wsum_slices(4, 65536, 16, false) == 3);
  CHECK(pol::wsum_slices(4, 65536, 2, false) == 2);                    // clamped to n_terms
  setenv("PGPU_WSUM_SLICES", "1", 1);
  CHECK(pol::wsum_slices(4, 1, 64, false) == 1);
  unsetenv("PGPU_WSUM_SLICES");
  // ---- the form ----
  {
    int G = 0, K = 0;
    CHECK(pol::wsum_geometry(1024, 100, &G, &K) && G == 2 && K == 19);
    CHECK(pol::wsum_geometry(3072, 100, &G, &K) && G == 8 && K == 14);
    CHECK(pol::wsum_geometry(2048, 8192, &G, &K) && G == 8 && K == 9);      // 1024 wavefronts of 8 chains: one per SIMD
    CHECK(pol::wsum_geometry(2048, 8193, &G, &K) && G == 4 && K == 18);
    CHECK(pol::wsum_geometry(2048, 1, &G, &K) && G == 8 && K == 9);
    CHECK(!pol::wsum_geometry(3212, 1, &G, &K));
    CHECK(!pol::wsum_geometry(4096, 1, &G, &K));
    CHECK(pol::wsum_wide_pays(8, 8192) && !pol::wsum_wide_pays(8, 8193));
    setenv("PGPU_WSUM_WIDE", "0", 1);
    CHECK(pol::wsum_geometry(2048, 1, &G, &K) && G == 4 && K == 18);
    setenv("PGPU_WSUM_WIDE", "1", 1);
    CHECK(pol::wsum_geometry(2048, 1000000, &G, &K) && G == 8 && K == 9);
    CHECK(pol::wsum_geometry(1024, 1, &G, &K) && G == 2 && K == 19);        // (no wide form to force)
    unsetenv("PGPU_WSUM_WIDE");
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
