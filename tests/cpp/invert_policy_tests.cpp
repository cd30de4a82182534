// CPU unit test of the plan of the batched inversion (pailliercryptolib_amd/csrc/policy.cpp: invert_*; pgpu_batch_ct_negate /
// pgpu_batch_ct_sub): the chunk rule, the level, launch and product counts, and the descriptors of every level -- read back
// out of the plan IMAGE, at the offsets the call hands to its kernels, and EXECUTED here on small integers modulo a prime,
// level by level in the order the call launches them: forward passes, the gather of the totals, one inversion, walks back.
// The result is compared with the inverse of every element.  Pure host logic -- built with g++ from policy.cpp alone, no
// device, no HIP call.  The rule is documented in DESIGN.md ("Ciphertext negation and subtraction").
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "policy.hpp"

namespace pol = pgpu::policy;
using pgpu::kSegscanNoCarry;
using pgpu::SegscanChunk;
static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      ++g_failed;                                                          \
      std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);          \
    }                                                                      \
  } while (0)

static const uint64_t P = 1000003;   // a prime: products of values below P stay below 2^40
static uint64_t power(uint64_t b, uint64_t e) {
  uint64_t r = 1;
  for (b %= P; e; e >>= 1, b = b * b % P)
    if (e & 1) r = r * b % P;
  return r;
}

// Executes a plan the way invert_batch (capi_aggregate.inc) launches it and checks what every plan must hold.
// chunk > 0: forced at every level (PGPU_INVERT_CHUNK); 0: the rule's own, level by level.
static void check_plan(size_t count, int chunk, int G = 4) {
  if (chunk) setenv("PGPU_INVERT_CHUNK", std::to_string(chunk).c_str(), 1);
  else unsetenv("PGPU_INVERT_CHUNK");
  pol::InvertPlan plan;
  pol::InvertImage img;
  pol::invert_plan(count, G, &plan);
  pol::invert_image(plan, &img);
  const size_t nl = plan.levels.size();
  CHECK(nl >= 1 && plan.chunk == plan.levels[0].chunk && plan.chunk == pol::invert_chunk(G, count));
  if (chunk) CHECK(plan.chunk == chunk);
  CHECK((int)nl == pol::invert_levels(G, count));
  CHECK((nl == 1) == (count <= (size_t)plan.chunk));
  CHECK(pol::invert_fits(G, count));
  CHECK(plan.products == pol::invert_products(count) && plan.products == 3 * (count - 1));
  CHECK(img.fwd_at.size() == nl && img.back_at.size() == nl && img.in_at.size() == nl && img.out_at.size() == nl);
  std::vector<uint64_t> x(count);
  for (size_t i = 0; i < count; ++i) x[i] = 2 + (i * 7919 + count * 31) % (P - 2);
  // scratch rows of the levels above the first: in and out of every level never share a row
  std::vector<int> owner(img.scratch_rows, -1);
  for (size_t l = 1; l < nl; ++l)
    for (size_t k = 0; k < 2 * plan.levels[l].n; ++k) {
      const size_t row = (k < plan.levels[l].n ? img.in_at[l] + k : img.out_at[l] + k - plan.levels[l].n);
      CHECK(row < img.scratch_rows && owner[row] == -1);
      if (row < img.scratch_rows) owner[row] = (int)l;
    }
  for (int o : owner) CHECK(o > 0);
  std::vector<std::vector<uint64_t>> in(nl), out(nl);
  std::vector<std::vector<int>> stores(nl);
  in[0] = x;
  size_t executed = 0, launches = 0;
  for (size_t l = 0; l < nl; ++l) {       // forward
    const auto& lv = plan.levels[l];
    const size_t n = lv.n, c = (size_t)lv.chunk;
    CHECK(lv.chunk == pol::invert_chunk(G, n) && (!chunk || lv.chunk == chunk));
    CHECK(n == in[l].size() && lv.fwd.size() == lv.back.size());
    CHECK(lv.fwd.size() == (n <= c ? 1 : (n + c - 1) / c));
    CHECK((l + 1 == nl) == (lv.fwd.size() == 1));
    // the descriptors as the kernels see them: out of the image
    CHECK(img.fwd_at[l] % 16 == 0 && img.back_at[l] % 16 == 0);
    CHECK(img.fwd_at[l] + lv.fwd.size() * sizeof(SegscanChunk) <= img.image.size());
    CHECK(img.back_at[l] + lv.back.size() * sizeof(SegscanChunk) <= img.image.size());
    const SegscanChunk* fwd = (const SegscanChunk*)(img.image.data() + img.fwd_at[l]);
    CHECK(!std::memcmp(fwd, lv.fwd.data(), lv.fwd.size() * sizeof(SegscanChunk)));
    out[l].assign(n, 0);
    stores[l].assign(n, 0);
    for (size_t j = 0; j < lv.fwd.size(); ++j) {
      const SegscanChunk& k = fwd[j];
      if (j) CHECK(fwd[j - 1].len >= k.len);                    // by len descending
      CHECK(k.carry == kSegscanNoCarry && k.len >= 1 && k.len <= (uint32_t)c && k.begin == j * c && k.begin + k.len <= n);
      if (k.begin + k.len > n) continue;
      uint64_t acc = in[l][k.begin];
      out[l][k.begin] = acc;
      ++stores[l][k.begin];
      for (uint32_t t = 1; t < k.len; ++t, ++executed) {
        acc = acc * in[l][k.begin + t] % P;
        out[l][k.begin + t] = acc;
        ++stores[l][k.begin + t];
      }
    }
    for (int w : stores[l]) CHECK(w == 1);                      // the pass covers every row exactly once
    if (n > 1) ++launches;
    if (l + 1 == nl) break;
    // the gather of the totals: `full` chains end chunk rows apart, the last one ends with the level
    const size_t full = n / c, next = plan.levels[l + 1].n;
    CHECK(next == lv.fwd.size() && (full == next || full + 1 == next));
    in[l + 1].assign(next, 0);
    for (size_t j = 0; j < full; ++j) in[l + 1][j] = out[l][(c - 1) + j * c];
    if (full < next) in[l + 1][full] = out[l][n - 1];
    for (size_t j = 0; j < next; ++j) CHECK(in[l + 1][j] == out[l][lv.fwd[j].begin + lv.fwd[j].len - 1]);
  }
  // the one inversion
  const size_t top = plan.levels[nl - 1].n;
  const uint64_t total = top == 1 ? in[nl - 1][0] : out[nl - 1][top - 1];
  std::vector<uint64_t> uploaded(1, power(total, P - 2));
  for (size_t l = nl; l-- > 0;) {         // walk back
    const auto& lv = plan.levels[l];
    const std::vector<uint64_t>& u = l + 1 < nl ? out[l + 1] : uploaded;
    const SegscanChunk* back = (const SegscanChunk*)(img.image.data() + img.back_at[l]);
    CHECK(!std::memcmp(back, lv.back.data(), lv.back.size() * sizeof(SegscanChunk)));
    std::vector<int> written(lv.n, 0);
    for (size_t j = 0; j < lv.back.size(); ++j) {
      const SegscanChunk& k = back[j];
      CHECK(k.begin == lv.fwd[j].begin && k.len == lv.fwd[j].len && k.carry == j && k.carry < u.size());
      if (k.carry >= u.size() || k.begin + k.len > lv.n) continue;
      uint64_t U = u[k.carry];
      for (uint32_t t = k.len - 1; t >= 1; --t, executed += 2) {
        CHECK(written[k.begin + t - 1] == 0);                   // row t - 1 still holds its running product
        const uint64_t inv = out[l][k.begin + t - 1] * U % P;
        U = U * in[l][k.begin + t] % P;
        out[l][k.begin + t] = inv;
        ++written[k.begin + t];
      }
      out[l][k.begin] = U;
      ++written[k.begin];
    }
    for (int w : written) CHECK(w == 1);
    ++launches;
    for (size_t i = 0; i < lv.n; ++i) CHECK(out[l][i] * in[l][i] % P == 1);   // every level inverts its input
  }
  CHECK(executed == plan.products);
  CHECK((int)launches == pol::invert_launches(G, count));
  CHECK(launches == (count == 1 ? 1 : 2 * nl));
  unsetenv("PGPU_INVERT_CHUNK");
}

int main() {
  for (int chunk : {2, 3, 8}) {
    const size_t c = (size_t)chunk;
    for (size_t count : {(size_t)1, (size_t)2, (size_t)3, (size_t)7, (size_t)8, (size_t)9, (size_t)64, (size_t)65, (size_t)300,
                         c - 1, c, c + 1, c * c, c * c + 1, c * c * c, c * c * c + 1})
      if (count) check_plan(count, chunk);
  }
  check_plan(4096, 512);
  check_plan(100000, 8);
  // ---- the rule's own chunks, level by level: pairs wherever a level cannot fill the chip ----
  for (int G : {2, 4, 8})
    for (size_t count : {(size_t)1, (size_t)2, (size_t)3, (size_t)9, (size_t)64, (size_t)65, (size_t)300, (size_t)2048, (size_t)65536, (size_t)300001})
      check_plan(count, 0, G);
  check_plan((size_t)1 << 20, 0, 4);                              // chains of 8, then pairs: 131072 -> 65536 -> ... -> 2
  // ---- levels, launches and products ----
  auto forced = [](int c) { setenv("PGPU_INVERT_CHUNK", std::to_string(c).c_str(), 1); };
  forced(8);
  CHECK(pol::invert_levels(4, 1) == 1 && pol::invert_levels(4, 8) == 1 && pol::invert_levels(4, 9) == 2);
  CHECK(pol::invert_levels(4, 64) == 2 && pol::invert_levels(4, 65) == 3);
  CHECK(pol::invert_launches(4, 1) == 1 && pol::invert_launches(4, 2) == 2 && pol::invert_launches(4, 65) == 6);
  forced(2);
  CHECK(pol::invert_levels(4, 9) == 4 && pol::invert_levels(4, 3) == 2);
  forced(3);
  CHECK(pol::invert_levels(4, 28) == 4);
  unsetenv("PGPU_INVERT_CHUNK");
  CHECK(pol::invert_products(1) == 0 && pol::invert_products(300) == 897);
  CHECK(pol::invert_levels(4, 1) == 1 && pol::invert_levels(4, 2) == 1 && pol::invert_levels(4, 3) == 2 && pol::invert_levels(4, 64) == 6);
  CHECK(pol::invert_levels(4, 65536) == 16 && pol::invert_launches(4, 65536) == 32);
  CHECK(pol::invert_levels(4, (size_t)1 << 20) == 18);            // 2^20 -> 2^17 chains of 8, then 17 levels of pairs
  // ---- the chunk rule: segscan_chunk's fill (carried over), the floor of 2 (measured) ----
  for (int G : {2, 4, 8}) {
    const size_t chains = pol::kSegscanWavesPerSimd * pol::kSimds * (64 / (size_t)G);
    CHECK(pol::invert_chunk(G, 1) == (int)pol::kInvertMinChunk && pol::invert_chunk(G, 300) == 2 && pol::invert_chunk(G, chains * 3 - 1) == 2);
    CHECK(pol::invert_chunk(G, chains * 8) == 8 && pol::invert_chunk(G, chains * 20) == 20 && pol::invert_chunk(G, chains * 20 + 5) == 20);
    for (size_t count : {(size_t)1, (size_t)64, (size_t)2048, (size_t)65536, (size_t)1 << 20, (size_t)1 << 26}) {
      const size_t c = (size_t)pol::invert_chunk(G, count);
      CHECK(c >= 2 && c <= pol::kInvertForcedMax);
      CHECK(c == pol::kInvertMinChunk || (count + c - 1) / c >= chains);      // above the floor the chains fill the chip
      CHECK(pol::invert_fits(G, count));
    }
  }
  CHECK(pol::invert_chunk(4, (size_t)1 << 20) == 8);              // 2^20 elements of a 2048-bit key: 131072 chains of 8
  // ---- the form of a level ----
  CHECK(pol::invert_wide_pays(8, 8192) && !pol::invert_wide_pays(8, 8193) && pol::invert_wide_pays(8, 1));
  setenv("PGPU_INVERT_WIDE", "0", 1);
  CHECK(!pol::invert_wide_pays(8, 1));
  setenv("PGPU_INVERT_WIDE", "1", 1);
  CHECK(pol::invert_wide_pays(8, (size_t)1 << 20));
  unsetenv("PGPU_INVERT_WIDE");
  // ---- what a descriptor cannot address ----
  forced(2);
  CHECK(!pol::invert_fits(4, (size_t)1 << 33) && pol::invert_fits(4, ((size_t)1 << 33) - 4));
  forced(8);
  CHECK(pol::invert_fits(4, (size_t)1 << 34));
  forced(65536);
  CHECK(!pol::invert_fits(4, ~(size_t)0 / 2));
  unsetenv("PGPU_INVERT_CHUNK");
  // ---- the forced knob (read at every call) ----
  const int dflt = pol::invert_chunk(4, (size_t)1 << 21);
  CHECK(dflt == 16);
  setenv("PGPU_INVERT_CHUNK", "3", 1);
  CHECK(pol::invert_chunk(4, 4096) == 3 && pol::invert_chunk(2, (size_t)1 << 26) == 3);
  setenv("PGPU_INVERT_CHUNK", "100000", 1);
  CHECK(pol::invert_chunk(4, 5) == (int)pol::kInvertForcedMax);
  setenv("PGPU_INVERT_CHUNK", "1", 1);
  CHECK(pol::invert_chunk(4, (size_t)1 << 21) == dflt);          // below 2: ignored
  unsetenv("PGPU_INVERT_CHUNK");
  CHECK(pol::invert_chunk(4, (size_t)1 << 21) == dflt);
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
