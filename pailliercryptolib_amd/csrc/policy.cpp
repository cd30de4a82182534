// pailliercryptolib_amd -- kernel-form policy (policy.hpp).  Split out of capi.cpp in round 5; no behaviour change.
#include "policy.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "launch.hpp"

namespace pgpu {
namespace policy {

namespace {
int env_int(const char* name, int dflt, int lo, int hi) {
  const char* e = std::getenv(name);
  return e ? std::max(lo, std::min(hi, std::atoi(e))) : dflt;
}
// PGPU_SEQ_DECRYPT: 0 = never, 1 = for launches that put at least one wavefront of that form on every SIMD (16384
// ciphertexts under a 2048-bit key, 8192 under a 3072-bit key), 2 = whenever it applies.  hensel_seq.hpp: both halves of a
// residue in the same lanes, one after the other -- 10-13 % fewer instructions per exponentiation on half the lanes.
// 3: the round-3 opt-in mode for two batch lanes that are both kept busy -- a CRT decrypt also takes the form when it
// fills HALF the chip, its workgroups claiming more than half a CU's LDS so that the two lanes' launches spread over all
// CUs; every other operation as under 1.
// 4 (default since round 4): ADAPTIVE -- by launch size as under 1, and a launch that would leave SIMDs empty in this
// form takes it all the same when the GPU's OTHER batch lanes have work queued at launch time, i.e. when this launch
// will share the chip anyway: with b busy neighbours it needs waves * (1 + b) >= SIMDs, and claims the LDS that keeps
// a second workgroup off its CUs.  A lone caller -- nothing queued beside it -- keeps the full-chip paired kernels.  The
// probe is a hipStreamQuery per lane: what it costs when it is wrong is bounded by one launch (a neighbour that drains
// early leaves a half-chip launch to finish alone: 8.1 instead of 4.6 ms for 8192 ciphertexts).
std::atomic<int> g_seq_policy{env_int("PGPU_SEQ_DECRYPT", 4, 0, 4)};
// the one-lane product-scanning form (hensel_ps.hpp; 2048-bit keys).  64 exponentiations per wavefront: 8192 ciphertexts
// are 256 wavefronts -- a quarter of the SIMDs.  0 never; 1 (default) launches that put a wavefront on every SIMD that way
// (32768 ciphertexts), or -- adaptive, like the sequential-halves form -- do so together with the busy neighbour lanes:
// waves * (1 + busy) >= SIMDs (16384 ciphertexts beside one busy lane, 8192 beside three); 2 whenever compiled (tests)
std::atomic<int> g_ps_policy{env_int("PGPU_PS_DECRYPT", 1, 0, 2)};
// Two constants of the adaptive policy that were knobs (PGPU_ADAPT_ENC_SEQ / PGPU_ADAPT_CLAIM_BUSY) in rounds 4-5 and have
// sat at these values since: up to how many busy neighbours the DJN encrypt follows the decrypt into the sequential-halves
// form with a CU claim -- round 4 stopped at ONE (two lanes, each owning half the chip: 4.92 -> 4.87 ms per step); round 5:
// three, because beside one-lane decrypts a co-resident encrypt wavefront only gets the issue slots the older decrypt
// wavefront leaves (0.8 -> 10 ms), so the encrypt takes the lane's own quarter of the chip (capi.cpp: encrypt_on) -- and up
// to how many busy neighbours a part-chip launch claims whole CUs.
constexpr int kAdaptEncSeq = 3;
constexpr int kAdaptClaimBusy = 3;
// PGPU_RR_ADAPT = k > 0 (round 5; default 3): threads on ROUND-ROBIN lanes (synchronous callers of the ipcl:: API side by
// side) enter the adaptive policy as well, but only when at least k other lanes are active -- with all four lanes busy each
// caller's launches take a quarter of the chip (17 ms per encrypt + decrypt instead of 5.4 on the whole chip, four of them
// side by side: 5.3 against 5.9 ms per pair), which pays although every caller's quarter idles through its copies and host
// work; with one busy neighbour (half-chip forms) it does not (r04: 11.8 against 7.2 ms per pair).  0: lone-caller forms.
// PGPU_WAVE_FORMS: the latency forms (hensel_wave.hpp, hensel_wave_n2.hpp: one wavefront per exponentiation) -- 0 never,
// 1 (default) for small launches of a caller that has the chip to itself, 2 always where a kernel exists (tests)
std::atomic<int> g_wave_policy{env_int("PGPU_WAVE_FORMS", 1, 0, 2)};
std::atomic<int> g_rr_adapt{env_int("PGPU_RR_ADAPT", 3, 0, 100)};
// PGPU_PS_ODD_TABLE (default 1): the one-lane decrypt forms under the indexed table policy keep the ODD powers of the base only
// and place a window's product after w - ctz(digit) of its squarings (hensel_ps.hpp); 0 brings the half-squared table back
std::atomic<int> g_ps_odd_table{env_int("PGPU_PS_ODD_TABLE", 1, 0, 1)};
}  // namespace

int seq_policy() { return g_seq_policy.load(); }
void set_seq_policy(int p) { g_seq_policy.store(p < 0 ? 0 : (p > 4 ? 4 : p)); }
int ps_policy() { return g_ps_policy.load(); }
void set_ps_policy(int p) { g_ps_policy.store(p < 0 ? 0 : (p > 2 ? 2 : p)); }
int adapt_claim_busy() { return kAdaptClaimBusy; }
int wave_policy() { return g_wave_policy.load(); }
void set_wave_policy(int p) { g_wave_policy.store(p < 0 ? 0 : (p > 2 ? 2 : p)); }
int ps_odd_table() { return g_ps_odd_table.load(); }
int set_ps_odd_table(int on) { return g_ps_odd_table.exchange(on ? 1 : 0); }
int rr_adapt() { return g_rr_adapt.load(); }
int set_rr_adapt(int min_busy) { return g_rr_adapt.exchange(min_busy < 0 ? 0 : min_busy); }

int seq_policy_by_size() {
  const int p = g_seq_policy.load();
  return (p == 3 || p == 4) ? 1 : p;
}
bool seq_adaptive(size_t waves, int busy) {
  return g_seq_policy.load() == 4 && busy >= 1 && waves * (size_t)(1 + busy) >= kSimds;
}
unsigned adaptive_cu_claim(size_t waves, int busy_lanes) {
  return (g_seq_policy.load() == 4 && waves < kSimds && busy_lanes >= 1 && busy_lanes <= kAdaptClaimBusy) ? 84000u : 0u;
}

bool fb_encrypt_seq_pays(int H, int K, size_t count, int busy) {
  if (!pgpu::hensel_fb_encrypt_seq_has(H, K)) return false;
  const size_t ipw = 64 / (size_t)H;
  const size_t waves = (count + ipw - 1) / ipw;
  const int pol = seq_policy_by_size();
  // (adaptive: beside busy neighbour lanes the form of half the wavefronts -- and a sixth fewer multiply-accumulates --
  // also for launches that would not fill the chip alone; 4-lane groups only, see below for the others)
  // beside ONE neighbour (half the chip each) and beside THREE (a quarter each: the lane's own CUs between its one-lane
  // decrypts); beside two the lanes' sequential-halves decrypts hold every CU and the paired full-chip encrypt squeezes
  // in better than a launch that waits for whole CUs (k = 3 of the lane sweep: 4.9-5.1 against 5.2 ms per step)
  if (H == 4 && busy != 2 && busy <= kAdaptEncSeq && seq_adaptive(waves, busy)) return true;
  // (2-lane groups, 1024-bit keys: measured equal or behind the paired kernel at 65536 elements -- 1.04 against 1.02 ms,
  // 0.96 against 0.92 ms: 19 limbs per lane and the LDS staging leave no register room -- so only when forced)
  if (H == 2 && pol != 2) return false;
  // (8-lane groups pay two DPP moves per row broadcast: alone on a SIMD the form is 2 % behind the paired kernel --
  // 3072-bit keys, 8192 elements: 3.60 against 3.52 ms -- and 7 % ahead with two wavefronts per SIMD: 6.2 against 6.7 ms)
  return pol == 2 || (pol == 1 && waves >= (H >= 8 ? 2 : 1) * kSimds);
}
bool modexp_seq_form_pays(int H, int K, size_t count) {
  if (!pgpu::hensel_modexp_seq_has(H, K)) return false;
  const size_t ipw = 64 / (size_t)H;
  const size_t waves = (count + ipw - 1) / ipw;
  const int pol = seq_policy_by_size();
  if (H == 2 && pol != 2) return false;   // (see fb_encrypt_seq_pays)
  return pol == 2 || (pol == 1 && waves >= (H >= 8 ? 2 : 1) * kSimds);   // (8-lane groups: see fb_encrypt_seq_pays)
}
bool seq_form_pays(int H, int K, size_t count, int busy) {
  if (!pgpu::hensel_seq_has(H, K)) return false;
  const size_t ipw = 64 / (size_t)H;
  const size_t waves = 2 * ((count + ipw - 1) / ipw);
  const int pol = g_seq_policy.load();
  return pol == 2 || (pol == 3 && 2 * waves >= kSimds) || ((pol == 1 || pol == 4) && waves >= kSimds) || seq_adaptive(waves, busy);
}
// Measured on lone launches (profiles/r05_decrypt_partial_rounds.txt).  2048-bit keys (K = 38): a round 14.2 ms against
// 8.1 ms per 16384 ciphertexts of the sequential-halves form and 4.6 ms for up to 8192 in the paired one -- one round beats
// them above 16384 ciphertexts, and a tail of up to 16384 is cheaper as a launch of its own.  3072-bit keys (K = 56): a
// round 47.6 ms against 13.3-15.2 ms per 8192 of the (4,14) sequential-halves form: above 24576.  1024-bit keys (K = 19):
// a round 2.2-2.3 ms against 1.8 ms for 16384 ciphertexts and 3.0 ms for 24576 in the multi-lane forms: above 16384.
size_t ps_min_count(int K) {
  return K == 56 ? 24576 + 1 : (K == 38 || K == 19) ? 16384 + 1 : kPsRound;
}
static size_t ps_split_tail(int K) { return K == 56 ? 24576 : 16384; }
bool wave_form_pays(size_t count, int busy) {
  const int pol = g_wave_policy.load();
  if (pol == 2) return true;
  return pol == 1 && g_ps_policy.load() == 1 && busy == 0 && 2 * count <= kSimds;
}
bool modexp_wave_form_pays(size_t count) {
  const int pol = g_wave_policy.load();
  if (pol == 2) return true;
  return pol == 1 && g_ps_policy.load() == 1 && count <= kSimds;
}
bool ps_form_pays(size_t count, int busy, int K) {
  const size_t waves = 2 * ((count + 63) / 64);
  const int pol = g_ps_policy.load();
  return pol == 2 || (pol == 1 && (count >= ps_min_count(K) || seq_adaptive(waves, busy)));
}
size_t ps_split_head(int K, size_t count) {
  if (g_ps_policy.load() != 1 || count <= kPsRound) return 0;
  const size_t tail = count % kPsRound;
  return (tail != 0 && tail <= ps_split_tail(K)) ? count - tail : 0;
}
bool pair_mul_seq_pays(int H, int K, size_t count) {
  if (!pgpu::pair_mul_seq_has(H, K)) return false;
  const size_t ipw = 64 / (size_t)H;
  const size_t waves = (count + ipw - 1) / ipw;
  const int pol = seq_policy_by_size();
  return pol == 2 || (pol == 1 && waves >= (H >= 8 ? 2 : 1) * kSimds);   // (8-lane groups: see fb_encrypt_seq_pays)
}

// PGPU_FIXED_WINDOW=w: A/B measurements of the window width (what an LDS-resident table, which
// holds 8 entries per exponentiation at most, would have to beat); set_fixed_window: the same from a test, 0 = by the rules
static std::atomic<int> g_fixed_window{env_int("PGPU_FIXED_WINDOW", 0, 1, 6)};
int set_fixed_window(int w) { return g_fixed_window.exchange(w <= 0 ? 0 : std::min(w, 6)); }

int pick_window(int exp_bits) {
  const int forced = g_fixed_window.load();
  if (forced) return forced;
  int best = 1;
  long best_cost = 1L << 60;
  for (int w = 1; w <= 5; ++w) {
    long cost = ((1L << w) - 2) + (exp_bits + w - 1) / w;
    if (cost < best_cost) { best_cost = cost; best = w; }
  }
  return best;
}
// Window of the CRT-decrypt exponentiation (one secret exponent per side, shared by the launch): exponents of 1280 bits and
// more -- 3072-bit keys up -- also try w = 6 (1536 bits: 62 + 256 products instead of 30 + 308; 65536 ciphertexts 95.9 ->
// 94.7 ms).  Not for shorter ones: 1024 bits would tie on products and double the tables of the four-lane headline; and not
// in pick_window, whose per-element tables of a 1 M-element CT x PT would double with it.
// The window table of a launch is `entry_bytes` (all exponentiations of the launch, one entry each) x 2^w: w = 6 only while
// that stays under kDecryptTableCap -- a 65536-ciphertext launch of a 3072-bit key is 3.8 GB at w = 6 (config 4: kept), a
// 1 M-ciphertext one would be 60 GB for a gain of 1.2 %; entry_bytes = 0: no cap (the by-exponent rule alone).
//
// The ONE-LANE forms (hensel_ps.hpp, hensel_ps_bal.hpp) weigh the widths: a pair squaring is the cheaper of the two operations,
// the weights being the instructions of the two loops of hensel_decrypt_psb_kernel<36,29,1> (profiles/ps_balanced.txt; the
// unsigned kernels have the same ratio within 2 %: 5556 / 7844).  The rule is the least weighted count of the HALF-SQUARED
// table -- entry 2k = (entry k)^2, entry 2k+1 = entry 2k (x) base, the top digit's entry loaded directly: (nwin - 1) w +
// 2^(w-1) - 1 squarings and (nwin - 1) + 2^(w-1) - 1 products.  1024-bit exponents: 1035 + 219 at w = 5, 1051 + 201 at w = 6 --
// 7.04 M against 6.99 M instructions; 512 bits stay at 5 (3.61 M against 3.69 M), 1536 bits at 6.
// The ODD-POWER table (the default under indexed access, ps_odd_table()) has other counts (ps_one_lane_ops): one squaring and
// 2^(w-1) - 1 products build it, and every window -- the top one included, which starts from `one` -- is its bits' squarings
// and one product: exp_bits + 1 squarings WHATEVER the width, 2^(w-1) - 1 + nwin products.  Re-weighed with them, the widths
// of the rule above stand for every exponent class the one-lane kernels serve, so the rule is kept as it is and the width of
// a launch does not depend on the table form:
//   1024 bits: 1025 + 220 at w = 5, 1025 + 202 at w = 6, 1025 + 210 at w = 7 -- 6.87 M, 6.74 M, 6.80 M (5145 / 7278): 6.
//   1536 bits: 323 products at w = 5, 287 at w = 6, 283 at w = 7: 6; the seventh bit would save 0.3 % for twice the table (the
//     table fetch addresses 2^w entries and set_fixed_window stops at 6 as well).
//   512 bits: 118 products at w = 5, 117 at w = 6 -- one product in 3.5 M instructions (0.2 %) for twice the table, which the
//     window products of four lanes would then read from twice the footprint: stays at 5.
// (Where the two counts part is below these classes: a 256-bit exponent is 71 products at w = 4 and 67 at w = 5 in the odd
// form, 1.6 %, where the rule says 4.  tests/cpp/ps_odd_table_policy_tests.cpp holds the comparison.)
// The cap: the sixth bit is taken while 2^6 entries of the launch stay under kDecryptTableCap.  An odd-power table of w bits
// is as large as a full one of w - 1 bits plus one entry -- 8192 ciphertexts of a 2048-bit key are 156 MB at w = 6, 302 MB
// half-squared -- so the cap would admit one more bit; the threshold stays where it was, for the same reason as the rule.
// The multi-lane forms (sequential-halves, paired, wavefront-wide) build their tables with chained products in kernels of
// their own and keep the rule above.
constexpr size_t kDecryptTableCap = (size_t)4 << 30;
constexpr long kPsSqrInstr = 5260, kPsMulInstr = 7278;
void ps_one_lane_ops(int exp_bits, int w, bool odd, long* squarings, long* products) {
  const long nwin = (exp_bits + w - 1) / w, half = 1L << (w - 1);
  if (odd) {
    *squarings = (half > 1 ? 1 : 0) + exp_bits;
    *products = (half - 1) + nwin;
  } else {
    *squarings = (nwin - 1) * w + half - 1;
    *products = (nwin - 1) + half - 1;
  }
}
int pick_decrypt_window(int exp_bits, size_t entry_bytes, bool one_lane) {
  const int w5 = pick_window(exp_bits);
  if (g_fixed_window.load()) return w5;
  if (one_lane) {
    int best = 1;
    long best_cost = 1L << 60;
    for (int w = 1; w <= 6; ++w) {
      if (w == 6 && entry_bytes > (kDecryptTableCap >> 6)) break;   // (the cap is on the sixth bit, as below)
      long sq, mu;
      ps_one_lane_ops(exp_bits, w, false, &sq, &mu);
      const long cost = sq * kPsSqrInstr + mu * kPsMulInstr;
      if (cost < best_cost) { best_cost = cost; best = w; }
    }
    return best;
  }
  if (exp_bits < 1280) return w5;
  if (entry_bytes > (kDecryptTableCap >> 6)) return w5;
  const long c5 = ((1L << w5) - 2) + (exp_bits + w5 - 1) / w5, c6 = ((1L << 6) - 2) + (exp_bits + 5) / 6;
  return c6 < c5 ? 6 : w5;
}
// Window of the CRT-decrypt exponentiation under the masked table gather (round 5): every one of the 2^w entries of an
// exponentiation's table is read at every window product, so the table is what the launch streams -- 9.7 KB per
// exponentiation at w = 5, 32 entries x 235 products; four batches in flight (636 MB of tables) fall out of the 256 MB
// Infinity Cache and the one-lane decrypt went from 14.5 to 41 ms.  w = 3: 8 entries x 348 products, a third of the bytes,
// 11 % more products: 26 ms (lone paired launch: 6.6 -> 6.0 ms against 4.6 indexed).
int masked_decrypt_window() { return 3; }

// ---- encrypted matrix-vector product ----
// (the knobs are read at every call, not once: a test process walks through several forced shapes)
static long env_now(const char* name) {
  const char* e = std::getenv(name);
  return e && *e ? std::atol(e) : 0;
}
bool pair_form_for_bits(int n_bits, int* G, int* K) {
  // R = 2^(29 G K) >= 2^8 P with P = n k < 2^(bits + 29); from fewest lanes to most, and of one lane count the fewest limbs
  static const int forms[4][2] = {{2, 19}, {4, 18}, {8, 14}, {8, 18}};
  if (n_bits < 1) return false;
  for (const auto& f : forms) {
    if (pgpu::kLimbBits * f[0] * f[1] >= n_bits + pgpu::kLimbBits + 8 && pgpu::pair_ops_has(f[0], f[1])) {
      if (G) *G = f[0];
      if (K) *K = f[1];
      return true;
    }
  }
  return false;
}
bool pair_wide_form(int G, int K, int* wide_G, int* wide_K) {
  if (K % 2 != 0 || !pgpu::pair_ops_alt_has(2 * G, K / 2)) return false;
  if (wide_G) *wide_G = 2 * G;
  if (wide_K) *wide_K = K / 2;
  return true;
}
void pub_forms_for_bits(int n_bits, std::vector<std::pair<int, int>>* forms) {
  forms->clear();
  if (n_bits < 1) return;
  const int need = n_bits + pgpu::kLimbBits + 8, nsq_bits = 2 * n_bits;
  int PG = 0, PK = 0, WG = 0, WK = 0;
  const bool has_pair = pair_form_for_bits(n_bits, &PG, &PK);
  const bool has_wide = has_pair && pair_wide_form(PG, PK, &WG, &WK);
  for (int H : {8, 4, 2})
    for (int K = 1; K <= 19; ++K)
      if ((pgpu::hensel_modexp_has(H, K) || pgpu::hensel_fb_has(H, K)) && pgpu::kLimbBits * H * K >= need &&
          2 * pgpu::kLimbBits * H * K >= nsq_bits + 8) {
        if (!(has_pair && H == PG && K == PK) && !(has_wide && H == WG && K == WK)) forms->push_back({H, K});
        break;
      }
  if (has_wide) forms->push_back({WG, WK});
  if (has_pair) forms->push_back({PG, PK});
}
bool matvec_geometry(int key_bits, int* G, int* K) {
  int g = 0, k = 0;
  if (!pair_form_for_bits(key_bits, &g, &k) || !pgpu::matvec_has(g, k)) return false;
  if (G) *G = g;
  if (K) *K = k;
  return true;
}
size_t matvec_slices(int G, size_t rows, size_t cols) {
  if (rows == 0 || cols == 0) return 1;
  const long forced = env_now("PGPU_MATVEC_SLICES");
  if (forced > 0) return std::min((size_t)forced, cols);
  const size_t ipw = 64 / (size_t)G;
  const size_t row_waves = (rows + ipw - 1) / ipw;               // wavefronts of one slice
  const size_t fill = (kSimds + row_waves - 1) / row_waves;      // slices that put a wavefront on every SIMD
  const size_t cap = std::max<size_t>(1, cols / kMatvecMinSliceCols);
  return std::max<size_t>(1, std::min(std::min(fill, cap), cols));
}
double matvec_products(size_t rows, size_t cols, int e_bits, int w, size_t slices) {
  const double nwin = (double)((e_bits + w - 1) / w);
  return (double)cols * (double)(((size_t)1 << w) - 2) + (double)rows * (double)slices * (double)e_bits +
         (double)rows * (double)cols * nwin + (double)rows * (double)(slices - 1);
}
int matvec_window(size_t rows, size_t cols, int e_bits, size_t slices, size_t row_bytes) {
  const long forced = env_now("PGPU_MATVEC_WINDOW");
  if (forced > 0) return (int)std::min(forced, 6L);
  int best = 1;
  double best_cost = matvec_products(rows, cols, e_bits, 1, slices);
  for (int w = 2; w <= 6; ++w) {
    if ((double)cols * (double)((size_t)1 << w) * (double)row_bytes > (double)kMatvecTableCap) break;
    const double cost = matvec_products(rows, cols, e_bits, w, slices);
    if (cost < best_cost) { best_cost = cost; best = w; }
  }
  return best;
}


// ---- encrypted matrix product ----
// the matvec's slice rule without its knob (matvec_slices above: the same four lines)
static size_t slices_rule(int G, size_t rows, size_t cols) {
  const size_t ipw = 64 / (size_t)G;
  const size_t row_waves = (rows + ipw - 1) / ipw;
  const size_t fill = (kSimds + row_waves - 1) / row_waves;
  const size_t cap = std::max<size_t>(1, cols / kMatvecMinSliceCols);
  return std::max<size_t>(1, std::min(std::min(fill, cap), cols));
}
// a tiled call -- n items (vectors, images) of `elems` table elements each, `rows` outputs per item over `cols` terms -- for
// both the matrix product (elems == cols) and the convolution (elems = c_in*h*w, cols = taps)
static size_t tiled_slices_with(long forced, int G, size_t t, size_t rows, size_t cols) {
  if (forced > 0) return std::min((size_t)forced, cols);
  return slices_rule(G, t * rows, cols);
}
static double tiled_products_with(long forced_s, int G, size_t n, size_t elems, size_t rows, size_t cols, int e_bits, int w, size_t tile) {
  const double nwin = (double)((e_bits + w - 1) / w);
  const auto pass = [&](size_t t) {
    const double S = (double)tiled_slices_with(forced_s, G, t, rows, cols), out = (double)t * (double)rows;
    return (double)t * (double)elems * (double)(((size_t)1 << w) - 2) + out * S * (double)e_bits + out * (double)cols * nwin + out * (S - 1);
  };
  const size_t full = n / tile, rem = n % tile;
  return (double)full * pass(tile) + (rem ? pass(rem) : 0.0);
}
// (extra_rows: rows of an element's table beyond 2^w -- 0, or 1 for the signed calls' tables over [x ; x^-1]; only the cap sees them)
static void tiled_plan_with(long fw, long ft, long fs, int G, size_t n, size_t elems, size_t rows, size_t cols, int e_bits,
                            size_t row_bytes, size_t extra_rows, MatmulPlan* plan) {
  const int w_lo = fw > 0 ? (int)std::min(fw, 6L) : 1, w_hi = fw > 0 ? w_lo : 6;
  int best_w = w_lo;
  size_t best_t = ft > 0 ? std::min((size_t)ft, n) : 1;
  double best_cost = -1;
  for (int w = w_lo; w <= w_hi; ++w) {
    // items whose tables fit the cap at this window; a forced value is taken as it is
    size_t t_hi = 0;
    if (elems <= kMatvecTableCap) t_hi = std::min(n, kMatvecTableCap / (elems * (((size_t)1 << w) + extra_rows) * row_bytes));
    if (t_hi == 0) {
      if (w > w_lo) break;
      t_hi = 1;     // one oversized item: tile = 1 at the smallest window
    }
    size_t t_lo = 1;
    if (ft > 0) t_lo = t_hi = std::min((size_t)ft, n);
    for (size_t t = t_hi; t >= t_lo; --t) {
      const double cost = tiled_products_with(fs, G, n, elems, rows, cols, e_bits, w, t);
      // ties: the larger tile, then the smaller window
      if (best_cost < 0 || cost < best_cost || (cost == best_cost && (t > best_t || (t == best_t && w < best_w)))) {
        best_cost = cost;
        best_w = w;
        best_t = t;
      }
    }
  }
  plan->window = best_w;
  plan->tile = best_t;
  plan->passes = (n + best_t - 1) / best_t;
  plan->last = n - (plan->passes - 1) * best_t;
  plan->slices = tiled_slices_with(fs, G, best_t, rows, cols);
  plan->last_slices = tiled_slices_with(fs, G, plan->last, rows, cols);
  plan->products = best_cost;
}
size_t matmul_slices(int G, size_t t, size_t rows, size_t cols) {
  if (t == 0 || rows == 0 || cols == 0) return 1;
  return tiled_slices_with(env_now("PGPU_MATMUL_SLICES"), G, t, rows, cols);
}
double matmul_products(int G, size_t n_vec, size_t rows, size_t cols, int e_bits, int w, size_t tile) {
  return tiled_products_with(env_now("PGPU_MATMUL_SLICES"), G, n_vec, cols, rows, cols, e_bits, w, tile);
}
void matmul_plan(int G, size_t n_vec, size_t rows, size_t cols, int e_bits, size_t row_bytes, MatmulPlan* plan) {
  tiled_plan_with(env_now("PGPU_MATMUL_WINDOW"), env_now("PGPU_MATMUL_TILE"), env_now("PGPU_MATMUL_SLICES"), G, n_vec, cols, rows,
                  cols, e_bits, row_bytes, 0, plan);
}


// ---- signed-weight matvec and matmul ----
// the unsigned counts (a signed table of 2h + 1 rows costs 2 (h - 1) = 2^w - 2 products, the Booth recoding has the same
// ceil(e_bits / w) digits) plus the inversion; the table is one row longer per element, which only the cap sees
double matvec_signed_products(size_t rows, size_t cols, int e_bits, int w, size_t slices) {
  return matvec_products(rows, cols, e_bits, w, slices) + (double)invert_products(cols);
}
int matvec_signed_window(size_t rows, size_t cols, int e_bits, size_t slices, size_t row_bytes) {
  const long forced = env_now("PGPU_MATVEC_WINDOW");
  if (forced > 0) return (int)std::min(forced, 6L);
  int best = 1;
  double best_cost = matvec_products(rows, cols, e_bits, 1, slices);
  for (int w = 2; w <= 6; ++w) {
    if ((double)cols * (double)(((size_t)1 << w) + 1) * (double)row_bytes > (double)kMatvecTableCap) break;
    const double cost = matvec_products(rows, cols, e_bits, w, slices);
    if (cost < best_cost) { best_cost = cost; best = w; }
  }
  return best;
}
void matmul_signed_plan(int G, size_t n_vec, size_t rows, size_t cols, int e_bits, size_t row_bytes, MatmulPlan* plan) {
  // tiled_plan_with over tables of 2^w + 1 rows per element
  tiled_plan_with(env_now("PGPU_MATMUL_WINDOW"), env_now("PGPU_MATMUL_TILE"), env_now("PGPU_MATMUL_SLICES"), G, n_vec, cols, rows,
                  cols, e_bits, row_bytes, 1, plan);
  // the one inversion runs over all n_vec * cols elements before the first pass
  plan->products += (double)invert_products(n_vec * cols);
}


// ---- encrypted 2-D convolution ----
// the matrix product's plan with the table of an item (an image's c_in*h*w elements) apart from the terms of an output
// (its c_in*kh*kw taps)
size_t conv_slices(int G, size_t t, size_t n_o, size_t taps) {
  if (t == 0 || n_o == 0 || taps == 0) return 1;
  return tiled_slices_with(env_now("PGPU_CONV_SLICES"), G, t, n_o, taps);
}
double conv_products(int G, size_t n_img, size_t elems, size_t n_o, size_t taps, int e_bits, int w, size_t tile) {
  return tiled_products_with(env_now("PGPU_CONV_SLICES"), G, n_img, elems, n_o, taps, e_bits, w, tile);
}
void conv_plan(int G, size_t n_img, size_t elems, size_t n_o, size_t taps, int e_bits, size_t row_bytes, ConvPlan* plan) {
  tiled_plan_with(env_now("PGPU_CONV_WINDOW"), env_now("PGPU_CONV_TILE"), env_now("PGPU_CONV_SLICES"), G, n_img, elems, n_o,
                  taps, e_bits, row_bytes, 0, plan);
}
// the signed call: conv_plan over tables of 2^w + 1 rows per element, plus the one inversion of all n_img * elems elements
void conv_signed_plan(int G, size_t n_img, size_t elems, size_t n_o, size_t taps, int e_bits, size_t row_bytes, ConvPlan* plan) {
  tiled_plan_with(env_now("PGPU_CONV_WINDOW"), env_now("PGPU_CONV_TILE"), env_now("PGPU_CONV_SLICES"), G, n_img, elems, n_o,
                  taps, e_bits, row_bytes, 1, plan);
  plan->products += (double)invert_products(n_img * elems);
}
bool conv_geometry(const size_t d[11], ConvDims* g) {
  const size_t n_img = d[0], c_in = d[1], h = d[2], w = d[3], c_out = d[4], kh = d[5], kw = d[6], sh = d[7], sw = d[8], ph = d[9], pw = d[10];
  constexpr size_t kSide = (size_t)1 << 30;
  if (!n_img || !c_in || !h || !w || !c_out || !kh || !kw || !sh || !sw) return false;
  if (ph >= kh || pw >= kw) return false;
  if (h >= kSide || w >= kSide || kh >= kSide || kw >= kSide) return false;
  if (kh > h + 2 * ph || kw > w + 2 * pw) return false;
  const auto mul = [](size_t a, size_t b, size_t* r) {
    if (a && b > ~(size_t)0 / a) return false;
    *r = a * b;
    return true;
  };
  g->oh = (h + 2 * ph - kh) / sh + 1;
  g->ow = (w + 2 * pw - kw) / sw + 1;
  size_t hw = h * w, kk = kh * kw, oo = g->oh * g->ow, wts, tmp;
  if (!mul(c_in, hw, &g->elems) || !mul(n_img, g->elems, &g->x_count)) return false;
  if (!mul(c_in, kk, &g->taps) || !mul(c_out, g->taps, &wts)) return false;
  if (!mul(c_out, oo, &g->n_o) || !mul(n_img, g->n_o, &g->out_count)) return false;
  // the sizes the call allocates and addresses in bytes: tables (64 entries of at most 2^11 bytes) and partial blocks
  if (!mul(g->x_count, (size_t)1 << 17, &tmp) || !mul(g->out_count, g->taps, &tmp) || !mul(tmp, (size_t)1 << 11, &tmp)) return false;
  // (the kernel carries channel and tap numbers in 32 bits)
  if (c_in >= ((size_t)1 << 31) || c_out >= ((size_t)1 << 31) || g->taps >= ((size_t)1 << 31)) return false;
  g->w_count = wts;
  return true;
}


// ---- encrypted segmented sum ----
bool segsum_sort(const uint32_t* ids, size_t groups, size_t cols, size_t n_segments, std::vector<uint32_t>* perm,
                 std::vector<size_t>* offsets) {
  const size_t segments = groups * n_segments;
  std::vector<size_t> off(segments + 1, 0);
  for (size_t g = 0; g < groups; ++g)
    for (size_t j = 0; j < cols; ++j) {
      const uint32_t id = ids[g * cols + j];
      if (id == kSegsumNone) continue;
      if (id >= n_segments) return false;
      ++off[g * n_segments + id + 1];
    }
  for (size_t s = 0; s < segments; ++s) off[s + 1] += off[s];
  std::vector<uint32_t> p(off[segments]);
  std::vector<size_t> next(off.begin(), off.end() - 1);
  for (size_t g = 0; g < groups; ++g)
    for (size_t j = 0; j < cols; ++j) {   // rising j: equal ids keep their order
      const uint32_t id = ids[g * cols + j];
      if (id != kSegsumNone) p[next[g * n_segments + id]++] = (uint32_t)j;
    }
  perm->swap(p);
  offsets->swap(off);
  return true;
}
int segsum_chunk(int G, size_t elements) {
  const long forced = env_now("PGPU_SEGSUM_CHUNK");
  if (forced >= 2) return (int)std::min(forced, (long)kSegsumForcedMax);
  const size_t chains = kSegsumWavesPerSimd * kSimds * (64 / (size_t)G);   // chains that fill the chip
  return (int)std::max(kSegsumMinChunk, std::min(kSegsumMaxChunk, elements / chains));
}
bool segsum_wide_pays(int wide_G, size_t chains) {
  const size_t ipw = 64 / (size_t)wide_G;
  return (chains + ipw - 1) / ipw <= kSimds;
}
int segsum_levels(int chunk, size_t longest) {
  int levels = 1;
  for (size_t m = longest; m > (size_t)chunk; m = (m + (size_t)chunk - 1) / (size_t)chunk) ++levels;
  return levels;
}
void segsum_plan(const std::vector<size_t>& offsets, int chunk, SegsumPlan* plan) {
  const size_t segments = offsets.empty() ? 0 : offsets.size() - 1, c = (size_t)chunk;
  plan->chunk = chunk;
  plan->longest = 0;
  plan->levels.clear();
  // the lists still to be multiplied: at level 0 the ranges of perm, afterwards ranges of the partial rows just written
  struct List { size_t seg, begin, len; };
  std::vector<List> todo;
  for (size_t s = 0; s < segments; ++s) {
    todo.push_back({s, offsets[s], offsets[s + 1] - offsets[s]});
    plan->longest = std::max(plan->longest, offsets[s + 1] - offsets[s]);
  }
  while (!todo.empty()) {
    SegsumLevel lv;
    std::vector<List> next;
    for (const List& l : todo) {
      if (l.len <= c) {
        lv.chunks.push_back({(uint64_t)l.begin, (uint32_t)l.len, (uint32_t)l.seg});
        continue;
      }
      const size_t parts = (l.len + c - 1) / c;
      next.push_back({l.seg, lv.partial_rows, parts});
      for (size_t k = 0; k < parts; ++k)
        lv.chunks.push_back({(uint64_t)(l.begin + k * c), (uint32_t)std::min(c, l.len - k * c),
                             kSegsumPartial | (uint32_t)(lv.partial_rows + k)});
      lv.partial_rows += parts;
    }
    // by len descending, equal lengths in the order made above: a counting sort (len <= chunk <= kSegsumForcedMax)
    {
      std::vector<size_t> at(c + 2, 0);
      for (const SegsumChunk& k : lv.chunks) ++at[c - k.len + 1];
      for (size_t i = 0; i <= c; ++i) at[i + 1] += at[i];
      std::vector<SegsumChunk> sorted(lv.chunks.size());
      for (const SegsumChunk& k : lv.chunks) sorted[at[c - k.len]++] = k;
      lv.chunks.swap(sorted);
    }
    plan->levels.push_back(std::move(lv));
    todo.swap(next);
  }
}


// ---- bucket-method encrypted matvec ----
int bucket_default_block(int c) { return 1 << ((c + 1) / 2); }
int bucket_log2(size_t v) {
  int l = 0;
  while (((size_t)1 << (l + 1)) <= v) ++l;
  return l;
}
double bucket_products(size_t rows, size_t cols, int e_bits, int c, int b) {
  const double W = (double)((e_bits + c - 1) / c), nb = (double)(((size_t)1 << c) / (size_t)b), r = (double)rows;
  return r * W * (double)cols + r * W * nb * 2.0 * (double)(b - 1) +
         r * W * (2.0 * (nb - 1) + (double)bucket_log2((size_t)b) + nb) + r * (W - 1) * (double)(c + 1);
}
size_t bucket_depth(int G, size_t rows, size_t cols, int e_bits, int c, int b) {
  const size_t W = (size_t)((e_bits + c - 1) / c), nb = ((size_t)1 << c) / (size_t)b;
  const size_t groups = rows > ~(size_t)0 / W ? ~(size_t)0 : rows * W;
  const size_t chunk = (size_t)segsum_chunk(G, cols && groups > ~(size_t)0 / cols ? ~(size_t)0 : groups * cols);
  size_t depth = 0;
  for (size_t m = cols;; m = (m + chunk - 1) / chunk) {
    depth += std::min(chunk, m);
    if (m <= chunk) break;
  }
  return depth + 2 * ((size_t)b - 1) + 2 * (nb - 1) + (size_t)bucket_log2((size_t)b) + nb + (W - 1) * (size_t)(c + 1);
}
void bucket_plan(int G, size_t rows, size_t cols, int e_bits, size_t row_bytes, BucketPlan* plan, double depth_weight) {
  const long fc = env_now("PGPU_BUCKET_WINDOW"), fb = env_now("PGPU_BUCKET_BLOCK");
  const int c_lo = fc > 0 ? (int)std::min(fc, (long)kBucketMaxWindow) : 1, c_hi = fc > 0 ? c_lo : kBucketMaxWindow;
  const double chains = (double)(kSimds * 2 * (64 / (size_t)G));
  int best_c = c_lo, best_b = 1;
  double best_cost = -1;
  for (int c = c_lo; c <= c_hi; ++c) {
    const double W = (double)((e_bits + c - 1) / c);
    // (a forced window is taken as it is; c = 1 stands in where no window fits the cap)
    if (fc <= 0 && c > 1 && (double)rows * W * (double)((size_t)1 << c) * (double)row_bytes > (double)kMatvecTableCap) continue;
    int b = bucket_default_block(c);
    if (fb > 0) b = 1 << bucket_log2((size_t)std::min(fb, 1L << c));
    const double cost = bucket_products(rows, cols, e_bits, c, b) / chains + depth_weight * (double)bucket_depth(G, rows, cols, e_bits, c, b);
    if (best_cost < 0 || cost < best_cost) {     // (rising c: ties stay with the smaller one)
      best_cost = cost;
      best_c = c;
      best_b = b;
    }
  }
  plan->window = best_c;
  plan->block = best_b;
  plan->windows = (size_t)((e_bits + best_c - 1) / best_c);
  plan->nb = ((size_t)1 << best_c) / (size_t)best_b;
  const double bytes = (double)rows * (double)plan->windows * (double)((size_t)1 << best_c) * (double)row_bytes;
  plan->bucket_bytes = bytes >= 18446744073709551615.0 ? ~(size_t)0 : (size_t)bytes;
  plan->products = bucket_products(rows, cols, e_bits, best_c, best_b);
  plan->depth = bucket_depth(G, rows, cols, e_bits, best_c, best_b);
}
// digit t of a weight: the bits c t .. min(c t + c, e_bits) - 1 (the top window may be narrower than c)
static inline uint32_t bucket_digit(const uint64_t* v, int e_bits, int c, size_t t) {
  const size_t lo = t * (size_t)c;
  const int width = (int)std::min((size_t)c, (size_t)e_bits - lo), sh = (int)(lo % 64);
  uint64_t d = v[lo / 64] >> sh;
  if (sh + width > 64) d |= v[lo / 64 + 1] << (64 - sh);   // (the word above exists: the digit ends below e_bits)
  return (uint32_t)(d & (((uint64_t)1 << width) - 1));
}
void bucket_sort(const uint64_t* w, int w_words, size_t rows, size_t cols, int e_bits, int c, std::vector<uint32_t>* perm,
                 std::vector<size_t>* offsets) {
  const size_t W = (size_t)((e_bits + c - 1) / c), nseg = (size_t)1 << c, segments = rows * W * nseg;
  std::vector<size_t> off(segments + 1, 0);
  for (size_t i = 0; i < rows; ++i)
    for (size_t j = 0; j < cols; ++j) {
      const uint64_t* v = w + (i * cols + j) * (size_t)w_words;
      for (size_t t = 0; t < W; ++t) {
        const uint32_t d = bucket_digit(v, e_bits, c, t);
        if (d) ++off[(i * W + t) * nseg + d + 1];
      }
    }
  for (size_t s = 0; s < segments; ++s) off[s + 1] += off[s];
  std::vector<uint32_t> p(off[segments]);
  std::vector<size_t> next(off.begin(), off.end() - 1);
  for (size_t i = 0; i < rows; ++i)
    for (size_t j = 0; j < cols; ++j) {   // rising j within every (row, window): equal digits keep their order
      const uint64_t* v = w + (i * cols + j) * (size_t)w_words;
      for (size_t t = 0; t < W; ++t) {
        const uint32_t d = bucket_digit(v, e_bits, c, t);
        if (d) p[next[(i * W + t) * nseg + d]++] = (uint32_t)j;
      }
    }
  perm->swap(p);
  offsets->swap(off);
}


// ---- encrypted sparse matrix-vector product ----
int spmv_chunk(int G, size_t nnz, size_t rows) {
  (void)rows;
  const long forced = env_now("PGPU_SPMV_CHUNK");
  if (forced >= 1) return (int)std::min(forced, (long)kSegsumForcedMax);
  const size_t chains = kSegsumWavesPerSimd * kSimds * (64 / (size_t)G);   // chains that fill the chip
  return (int)std::max(kSpmvMinChunk, std::min(kSpmvMaxChunk, nnz / chains));
}
// the chunk of the fold levels: the chains' own, but a fold by 1 would never end
static int spmv_fold_chunk(int chunk) { return std::max(2, chunk); }
int spmv_levels(int chunk, size_t longest) {
  const size_t c = (size_t)chunk;
  return longest <= c ? 1 : 1 + segsum_levels(spmv_fold_chunk(chunk), (longest + c - 1) / c);
}
bool spmv_plan(const uint64_t* row_ptr, size_t rows, int chunk, SpmvPlan* plan) {
  constexpr size_t kMax = (size_t)1 << 31;
  const size_t c = (size_t)chunk;
  if (!row_ptr || rows == 0 || rows >= kMax || chunk < 1 || row_ptr[0] != 0) return false;
  size_t n_chains = 0, longest = 0;
  for (size_t i = 0; i < rows; ++i) {
    if (row_ptr[i + 1] < row_ptr[i] || row_ptr[i + 1] >= kMax) return false;
    const size_t m = (size_t)(row_ptr[i + 1] - row_ptr[i]);
    n_chains += std::max<size_t>(1, (m + c - 1) / c);
    longest = std::max(longest, m);
    if (n_chains >= kMax) return false;
  }
  plan->chunk = chunk;
  plan->longest = longest;
  plan->partial_rows = 0;
  plan->chains.clear();
  plan->chains.reserve(n_chains);
  // the rows of several chains, as segments of the partial rows for the fold
  std::vector<size_t> fold_offsets(1, 0);
  std::vector<uint32_t> fold_row;
  for (size_t i = 0; i < rows; ++i) {
    const size_t begin = (size_t)row_ptr[i], m = (size_t)(row_ptr[i + 1] - row_ptr[i]);
    if (m <= c) {
      plan->chains.push_back({(uint64_t)begin, (uint32_t)m, (uint32_t)i});
      continue;
    }
    const size_t parts = (m + c - 1) / c;
    for (size_t k = 0; k < parts; ++k)
      plan->chains.push_back({(uint64_t)(begin + k * c), (uint32_t)std::min(c, m - k * c),
                              kSegsumPartial | (uint32_t)(plan->partial_rows + k)});
    plan->partial_rows += parts;
    fold_offsets.push_back(plan->partial_rows);
    fold_row.push_back((uint32_t)i);
  }
  plan->n_chains = plan->chains.size();
  // by len descending, equal lengths in the order made above: a counting sort (len <= chunk <= kSegsumForcedMax)
  {
    std::vector<size_t> at(c + 2, 0);
    for (const SegsumChunk& k : plan->chains) ++at[c - k.len + 1];
    for (size_t i = 0; i <= c; ++i) at[i + 1] += at[i];
    std::vector<SegsumChunk> sorted(plan->chains.size());
    for (const SegsumChunk& k : plan->chains) sorted[at[c - k.len]++] = k;
    plan->chains.swap(sorted);
  }
  // the fold: a segmented sum over the partial rows, segment s being row fold_row[s] of the result
  segsum_plan(fold_offsets, spmv_fold_chunk(chunk), &plan->fold);
  for (SegsumLevel& lv : plan->fold.levels)
    for (SegsumChunk& k : lv.chunks)
      if (!(k.dst & kSegsumPartial)) k.dst = fold_row[k.dst];
  return true;
}
double spmv_products(size_t rows, size_t cols, size_t nnz, size_t chains, int e_bits, int w) {
  const double nwin = (double)((e_bits + w - 1) / w);
  return (double)cols * (double)(((size_t)1 << w) - 2) + (double)chains * (double)e_bits + (double)nnz * nwin +
         (double)(chains - std::min(chains, rows));
}
// (extra_rows: rows of a column's table beyond 2^w -- 0, or 1 for the signed call's tables over [x ; x^-1]; only the cap sees them)
static int spmv_window_with(size_t extra_rows, size_t rows, size_t cols, size_t nnz, size_t chains, int e_bits, size_t row_bytes) {
  const long forced = env_now("PGPU_SPMV_WINDOW");
  if (forced > 0) return (int)std::min(forced, 6L);
  int best = 1;
  double best_cost = spmv_products(rows, cols, nnz, chains, e_bits, 1);
  for (int w = 2; w <= 6; ++w) {
    if ((double)cols * (double)(((size_t)1 << w) + extra_rows) * (double)row_bytes > (double)kMatvecTableCap) break;
    const double cost = spmv_products(rows, cols, nnz, chains, e_bits, w);
    if (cost < best_cost) { best_cost = cost; best = w; }
  }
  return best;
}
int spmv_window(size_t rows, size_t cols, size_t nnz, size_t chains, int e_bits, size_t row_bytes) {
  return spmv_window_with(0, rows, cols, nnz, chains, e_bits, row_bytes);
}
// the signed call: the unsigned counts (the signed table costs the same 2^w - 2 products, the Booth recoding has the same
// digits) plus the inversion of EVERY column of x; the table is one row longer per column, which only the cap sees
double spmv_signed_products(size_t rows, size_t cols, size_t nnz, size_t chains, int e_bits, int w) {
  return spmv_products(rows, cols, nnz, chains, e_bits, w) + (double)invert_products(cols);
}
int spmv_signed_window(size_t rows, size_t cols, size_t nnz, size_t chains, int e_bits, size_t row_bytes) {
  return spmv_window_with(1, rows, cols, nnz, chains, e_bits, row_bytes);
}
size_t spmv_chains_estimate(size_t rows, size_t nnz, size_t longest, int chunk) {
  const size_t c = (size_t)chunk, cut = [c](size_t m) { return std::max<size_t>(1, (m + c - 1) / c); }(longest);
  if (rows <= 1) return cut;
  const size_t rest = nnz > longest ? nnz - longest : 0, avg = (rest + rows - 2) / (rows - 1);
  return cut + (rows - 1) * std::max<size_t>(1, (avg + c - 1) / c);
}


// ---- encrypted segmented prefix sum ----
int segscan_chunk(int G, size_t rows, size_t seg_len) {
  const long forced = env_now("PGPU_SEGSCAN_CHUNK");
  if (forced >= 2) return (int)std::min(forced, (long)kSegscanForcedMax);
  const size_t whole = std::max<size_t>(1, std::min<size_t>(seg_len, (size_t)1 << 30));
  const size_t chains = kSegscanWavesPerSimd * kSimds * (64 / (size_t)G);   // chains that fill the chip
  if (rows >= chains || seg_len <= kSegscanMinChunk) return (int)whole;
  const size_t nchunks = (chains + std::max<size_t>(1, rows) - 1) / std::max<size_t>(1, rows);
  return (int)std::min(whole, std::max(kSegscanMinChunk, seg_len / nchunks));
}
int segscan_levels(int chunk, size_t seg_len) {
  const size_t c = (size_t)chunk;
  int levels = 1;
  for (size_t m = seg_len; m > c; m = (m + c - 1) / c - 1) ++levels;
  return levels;
}
size_t segscan_products(int chunk, size_t rows, size_t seg_len) {
  const size_t c = (size_t)chunk;
  size_t products = 0;
  for (size_t m = seg_len;; m = (m + c - 1) / c - 1) {
    products += rows * (m ? m - 1 : 0);
    if (m <= c) return products;
    products += rows * ((m + c - 1) / c - 1) * (c - 1);
  }
}
bool segscan_fits(int chunk, size_t rows, size_t seg_len) {
  const size_t c = (size_t)chunk, kMax = (size_t)1 << 31;
  if (seg_len && rows > ((size_t)1 << 62) / seg_len) return false;
  if (seg_len <= c) return seg_len < ((size_t)1 << 32);            // (len is a 32-bit field)
  return rows < kMax && (seg_len + c - 1) / c - 1 < kMax / std::max<size_t>(1, rows);
}
void segscan_plan(size_t rows, size_t seg_len, int chunk, bool reverse, SegscanPlan* plan) {
  const size_t c = (size_t)chunk;
  plan->chunk = chunk;
  plan->products = 0;
  plan->levels.clear();
  size_t m = seg_len;
  for (bool rev = reverse;; rev = false) {
    SegscanLevel lv;
    lv.rows = rows;
    lv.seg_len = m;
    lv.reverse = rev;
    const size_t nch = m <= c ? 1 : (m + c - 1) / c, head = std::min(c, m);
    lv.totals = rows * (nch - 1);
    // chunk k of a row in scan direction covers c entries from entry k * c of the scan; the lowest row of x among them
    for (size_t r = 0; r < rows; ++r)
      for (size_t k = 0; k + 1 < nch; ++k)
        lv.up.push_back({(uint64_t)(rev ? r * m + m - (k + 1) * c : r * m + k * c), (uint32_t)c,
                         kSegsumPartial | (uint32_t)(r * (nch - 1) + k)});
    plan->products += lv.totals * (c - 1);
    // by len descending: the whole chunks, then the last chunk of every row where it is shorter
    for (int pass = 0; pass < 2; ++pass)
      for (size_t r = 0; r < rows; ++r)
        for (size_t k = 0; k < nch; ++k) {
          const size_t len = std::min(c, m - k * c);
          if ((len == head) != (pass == 0)) continue;
          lv.scan.push_back({(uint64_t)(rev ? r * m + m - 1 - k * c : r * m + k * c), (uint32_t)len,
                             k ? (uint32_t)(r * (nch - 1) + k - 1) : kSegscanNoCarry});
        }
    plan->products += rows * (m - 1);
    plan->levels.push_back(std::move(lv));
    if (nch == 1) return;
    m = nch - 1;
  }
}


// ---- batched inversion ----
int invert_chunk(int G, size_t m) {
  const long forced = env_now("PGPU_INVERT_CHUNK");
  if (forced >= 2) return (int)std::min(forced, (long)kInvertForcedMax);
  const size_t chains = kSegscanWavesPerSimd * kSimds * (64 / (size_t)G);   // chains that fill the chip
  return (int)std::min(kInvertForcedMax, std::max(kInvertMinChunk, m / chains));
}
int invert_levels(int G, size_t count) {
  int levels = 1;
  for (size_t m = count;; ++levels) {
    const size_t c = (size_t)invert_chunk(G, m);
    if (m <= c) return levels;
    m = (m + c - 1) / c;
  }
}
int invert_launches(int G, size_t count) { return count <= 1 ? 1 : 2 * invert_levels(G, count); }
size_t invert_products(size_t count) { return count ? 3 * (count - 1) : 0; }
bool invert_fits(int G, size_t count) {
  const size_t c = (size_t)invert_chunk(G, count);
  if (count > ~(size_t)0 / 3) return false;
  return (count + c - 1) / c < (size_t)kSegscanNoCarry;
}
bool invert_wide_pays(int wide_G, size_t chains) {
  const char* e = std::getenv("PGPU_INVERT_WIDE");     // (unset is not 0 here: both values force)
  if (e && (e[0] == '0' || e[0] == '1') && !e[1]) return e[0] == '1';
  return segsum_wide_pays(wide_G, chains);
}
void invert_plan(size_t count, int G, InvertPlan* plan) {
  plan->chunk = invert_chunk(G, count);
  plan->products = 0;
  plan->levels.clear();
  for (size_t m = count;;) {
    InvertLevel lv;
    lv.n = m;
    lv.chunk = invert_chunk(G, m);
    const size_t c = (size_t)lv.chunk, nch = m <= c ? 1 : (m + c - 1) / c;
    lv.fwd.reserve(nch);
    lv.back.reserve(nch);
    for (size_t j = 0; j < nch; ++j) {
      const uint32_t len = (uint32_t)std::min(c, m - j * c);
      lv.fwd.push_back({(uint64_t)(j * c), len, kSegscanNoCarry});
      lv.back.push_back({(uint64_t)(j * c), len, (uint32_t)j});
    }
    plan->products += 3 * (m - nch);
    plan->levels.push_back(std::move(lv));
    if (nch == 1) return;
    m = nch;
  }
}


// ---- encrypted slot packing ----
bool pack_wide_pays(int wide_G, size_t rows) {
  const char* e = std::getenv("PGPU_PACK_WIDE");     // (unset is not 0 here: both values force)
  if (e && (e[0] == '0' || e[0] == '1') && !e[1]) return e[0] == '1';
  return segsum_wide_pays(wide_G, rows);
}
bool pack_geometry(int key_bits, size_t rows, int* G, int* K) {
  int g = 0, k = 0;
  if (!matvec_geometry(key_bits, &g, &k)) return false;
  // the form with the same limbs per half on twice the lanes, where one is compiled (capi_keys.inc builds it for such keys)
  if (k % 2 == 0 && pgpu::pack_wide_has(2 * g, k / 2) && pack_wide_pays(2 * g, rows)) {
    g *= 2;
    k /= 2;
  }
  if (G) *G = g;
  if (K) *K = k;
  return true;
}


// ---- encrypted weighted sum of K resident batches ----
size_t wsum_slices(int G, size_t count, size_t n_terms, bool unit_weights) {
  if (count == 0 || n_terms == 0) return 1;
  const long forced = env_now("PGPU_WSUM_SLICES");
  if (forced > 0) return std::min((size_t)forced, n_terms);
  const size_t ipw = 64 / (size_t)G;
  const size_t row_waves = (count + ipw - 1) / ipw;              // wavefronts of one slice
  const size_t fill = (kSimds + row_waves - 1) / row_waves;      // slices that put a wavefront on every SIMD
  const size_t cap = std::max<size_t>(1, n_terms / (unit_weights ? 2 : kMatvecMinSliceCols));
  return std::max<size_t>(1, std::min(std::min(fill, cap), n_terms));
}
bool wsum_wide_pays(int wide_G, size_t chains) {
  const char* e = std::getenv("PGPU_WSUM_WIDE");     // (unset is not 0 here: both values force)
  if (e && (e[0] == '0' || e[0] == '1') && !e[1]) return e[0] == '1';
  return segsum_wide_pays(wide_G, chains);
}
bool wsum_geometry(int key_bits, size_t chains, int* G, int* K) {
  int g = 0, k = 0;
  if (!matvec_geometry(key_bits, &g, &k)) return false;
  if (k % 2 == 0 && pgpu::wsum_wide_has(2 * g, k / 2) && wsum_wide_pays(2 * g, chains)) {
    g *= 2;
    k /= 2;
  }
  if (G) *G = g;
  if (K) *K = k;
  return true;
}
bool wsum_plan(const uint64_t* weights, int w_words, size_t n_terms, size_t S, WsumPlan* plan) {
  constexpr size_t kMax = (size_t)1 << 31;
  if (n_terms == 0 || n_terms > kWsumMaxTerms || S == 0 || (weights && w_words < 1)) return false;
  S = std::min(S, n_terms);
  const size_t ww = weights ? (size_t)w_words : 1;
  static const uint64_t kOne = 1;
  auto word = [&](size_t k, size_t j) -> uint64_t { return weights ? weights[k * ww + j] : kOne; };
  // bit length and popcount of every weight; then the step count of every slice, before anything is written
  std::vector<size_t> len(n_terms, 0), pop(n_terms, 0);
  for (size_t k = 0; k < n_terms; ++k)
    for (size_t j = 0; j < ww; ++j) {
      const uint64_t v = word(k, j);
      if (!v) continue;
      len[k] = 64 * j + (size_t)(64 - __builtin_clzll(v));
      pop[k] += (size_t)__builtin_popcountll(v);
    }
  struct Cut { size_t lo, hi, top, pops; };
  std::vector<Cut> cuts;
  for (size_t s = 0; s < S; ++s) {
    Cut c{s * n_terms / S, (s + 1) * n_terms / S, 0, 0};
    for (size_t k = c.lo; k < c.hi; ++k) {
      c.top = std::max(c.top, len[k]);
      c.pops += pop[k];
    }
    if (c.pops == 0) continue;                         // (every weight of the slice is zero: dropped)
    if (c.top - 1 + c.pops - 1 >= kMax) return false;
    cuts.push_back(c);
  }
  WsumPlan p;
  if (cuts.empty()) {
    p.all_zero = true;
    WsumSlice sl{};
    sl.first = sl.first_mul = kWsumNone;
    sl.term_end = (uint32_t)n_terms;
    p.slices.push_back(sl);
    *plan = std::move(p);
    return true;
  }
  for (const Cut& c : cuts) {
    WsumSlice sl{};
    sl.step_begin = p.steps.size();
    sl.first = sl.first_mul = kWsumNone;
    sl.term_begin = (uint32_t)c.lo;
    sl.term_end = (uint32_t)c.hi;
    size_t last_mul = (size_t)-1;                      // the MUL step whose `next` the coming MUL fills in
    for (size_t bit = c.top; bit-- > 0;) {
      if (bit != c.top - 1) {
        p.steps.push_back({kWsumSqr, kWsumNone});
        ++p.squarings;
      }
      for (size_t k = c.lo; k < c.hi; ++k) {
        if (!((word(k, bit >> 6) >> (bit & 63)) & 1)) continue;
        if (sl.first == kWsumNone) {                   // the load of the accumulator: no step
          sl.first = (uint32_t)k;
          continue;
        }
        if (last_mul == (size_t)-1) sl.first_mul = (uint32_t)k;
        else p.steps[last_mul].next = (uint32_t)k;
        last_mul = p.steps.size();
        p.steps.push_back({(uint32_t)k, kWsumNone});
        ++p.muls;
      }
    }
    sl.n_steps = (uint32_t)(p.steps.size() - sl.step_begin);
    p.longest = std::max(p.longest, (size_t)sl.n_steps);
    p.slices.push_back(sl);
  }
  p.products = p.squarings + p.muls + (p.slices.size() - 1);
  *plan = std::move(p);
  return true;
}


// ---- plan images ----
static_assert(sizeof(SegsumChunk) == 16 && sizeof(SegscanChunk) == 16, "descriptors are packed into one image behind a 16-byte boundary");
size_t PlanImage::add(const void* src, size_t n, size_t align) {
  const size_t at = (bytes.size() + align - 1) / align * align;
  bytes.resize(at + n, 0);
  if (src && n) std::memcpy(bytes.data() + at, src, n);
  return at;
}

void segsum_image(const std::vector<uint32_t>& perm, const SegsumPlan& plan, SegsumImage* out) {
  *out = SegsumImage();
  if (perm.empty()) out->image.add(nullptr, sizeof(uint32_t));
  else out->image.add(perm);
  for (size_t l = 0; l < plan.levels.size(); ++l) {
    out->level_at.push_back(out->image.add(plan.levels[l].chunks, l == 0 ? 16 : 1));
    out->region[l & 1] = std::max(out->region[l & 1], plan.levels[l].partial_rows);
  }
}

void spmv_image(const uint32_t* col_idx, size_t nnz, const SpmvPlan& plan, SpmvImage* out) {
  *out = SpmvImage();
  out->image.add(col_idx, nnz * sizeof(uint32_t));
  out->chains_at = out->image.add(plan.chains, 16);
  out->region[0] = plan.partial_rows;
  for (size_t f = 0; f < plan.fold.levels.size(); ++f) {
    out->fold_at.push_back(out->image.add(plan.fold.levels[f].chunks));
    out->region[(f + 1) & 1] = std::max(out->region[(f + 1) & 1], plan.fold.levels[f].partial_rows);
  }
}

void segscan_image(const SegscanPlan& plan, SegscanImage* out) {
  *out = SegscanImage();
  for (const SegscanLevel& lv : plan.levels) {
    out->up_at.push_back(out->image.add(lv.up));
    out->scan_at.push_back(out->image.add(lv.scan));
    out->totals_at.push_back(out->scratch_rows);
    out->carry_at.push_back(out->scratch_rows + lv.totals);
    out->scratch_rows += 2 * lv.totals;
  }
}

void invert_image(const InvertPlan& plan, InvertImage* out) {
  *out = InvertImage();
  for (size_t l = 0; l < plan.levels.size(); ++l) {
    const InvertLevel& lv = plan.levels[l];
    out->fwd_at.push_back(out->image.add(lv.fwd));
    out->back_at.push_back(out->image.add(lv.back));
    out->in_at.push_back(out->scratch_rows);
    out->out_at.push_back(out->scratch_rows + (l ? lv.n : 0));
    if (l) out->scratch_rows += 2 * lv.n;
  }
}

void wsum_image(const std::vector<const uint32_t*>& tab, const std::vector<const uint32_t*>& ftab, const WsumPlan& plan,
                const WsumPlan& fold, WsumImage* out) {
  *out = WsumImage();
  out->tab_at = out->image.add(tab);
  out->ftab_at = out->image.add(ftab);
  out->slices_at = out->image.add(plan.slices);
  out->fold_slices_at = out->image.add(fold.slices);
  out->steps_at = out->image.add(plan.steps);
  out->fold_steps_at = out->image.add(fold.steps);
}

// ---- gather, concat and slice of resident batches ----
bool gather_plan(size_t row_bytes, size_t n_out, GatherPlan* plan) {
  if (row_bytes == 0 || row_bytes % 8 != 0 || row_bytes > 0xFFFFFFFFull || n_out == 0) return false;
  GatherPlan p;
  p.vec_bytes = row_bytes % 16 == 0 ? 16 : 8;
  const size_t pieces = row_bytes / (size_t)p.vec_bytes;
  while ((1u << p.lanes_log2) < kGatherMaxLanes && ((size_t)1 << p.lanes_log2) < pieces) ++p.lanes_log2;
  p.lanes_per_row = 1 << p.lanes_log2;
  p.rows_per_wavefront = kWave / p.lanes_per_row;
  p.wavefronts = (n_out + (size_t)p.rows_per_wavefront - 1) / (size_t)p.rows_per_wavefront;
  p.blocks = (p.wavefronts + kWavesPerWG - 1) / kWavesPerWG;
  *plan = p;
  return true;
}

size_t gather_counts_ok(const size_t* counts, size_t n_src) {
  for (size_t k = 0; k < n_src; ++k)
    if (counts[k] >= kGatherMaxRows) return k;
  return n_src;
}

size_t gather_descs(const size_t* counts, size_t n_src, const uint64_t* idx, size_t n_out, std::vector<GatherDesc>* desc) {
  std::vector<uint64_t> end(n_src);   // end[k]: rows of sources 0..k
  uint64_t total = 0;
  for (size_t k = 0; k < n_src; ++k) end[k] = total += counts[k];
  desc->resize(n_out);
  size_t k = 0;                       // (the source of the previous index: neighbouring indices mostly share it)
  for (size_t i = 0; i < n_out; ++i) {
    const uint64_t v = idx[i];
    if (v == kGatherOne) {
      (*desc)[i] = GatherDesc{0u, kGatherOneRow};
      continue;
    }
    if (v >= total) return i;
    if (v >= end[k] || (k && v < end[k - 1])) k = (size_t)(std::upper_bound(end.begin(), end.end(), v) - end.begin());
    (*desc)[i] = GatherDesc{(uint32_t)k, (uint32_t)(v - (k ? end[k - 1] : 0))};
  }
  return n_out;
}

void gather_slice_descs(size_t start, size_t count, size_t step, std::vector<GatherDesc>* desc) {
  desc->resize(count);
  for (size_t i = 0; i < count; ++i) (*desc)[i] = GatherDesc{0u, (uint32_t)(start + i * step)};
}

void gather_image(const std::vector<const char*>& bases, const void* one, size_t row_bytes, const std::vector<GatherDesc>& desc,
                  GatherImage* out) {
  *out = GatherImage();
  out->bases_at = out->image.add(bases);
  out->one_at = out->image.add(one, row_bytes, 16);
  out->desc_at = out->image.add(desc, 8);
}

}  // namespace policy
}  // namespace pgpu
