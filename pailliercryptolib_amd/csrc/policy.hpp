// pailliercryptolib_amd -- the kernel-FORM policy of the host runtime: which form of a split-form kernel a launch takes,
// from its size and from what the GPU's other batch lanes are doing.  Pure host logic (sizes x busy lanes -> form, LDS
// claim, window): no device, no HIP call -- tests/cpp/policy_tests.cpp checks it on the CPU.  The measurements behind
// every threshold are in DESIGN.md sections 3-4; the environment knobs are read once.
//
// The forms (include/pgpu.h: pgpu_kernel_form; reference: the operations of ipcl/pri_key.cpp:114-146, pub_key.cpp:51-129,
// ciphertext.cpp:135-162 all funnel into one exponentiation primitive, which is what takes these forms here):
//   paired        hensel.hpp      the two halves of a residue in neighbouring lanes -- most lanes per residue: a lone caller
//   sequential    hensel_seq.hpp  both halves in the same lanes -- half the wavefronts: launches that still cover the SIMDs,
//                                 alone or together with one busy neighbour lane (each launch then claims half the chip)
//   one-lane      hensel_ps.hpp   a whole exponentiation per lane (product scanning) -- a quarter of the wavefronts again:
//                                 large launches, or 8192-ciphertext launches beside three busy lanes (a quarter chip each)
#ifndef PAILLIERCRYPTOLIB_AMD_CSRC_POLICY_HPP_
#define PAILLIERCRYPTOLIB_AMD_CSRC_POLICY_HPP_

#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "gather.hpp"
#include "kargs.hpp"

namespace pgpu {
namespace policy {

constexpr size_t kSimds = 256 * 4;   // MI355X: 256 CUs x 4 SIMDs; a launch of fewer wavefronts leaves SIMDs empty
// threads on round-robin lanes enter the adaptive policy only with launches of at least this many elements (capi.cpp:
// busy_other_lanes)
constexpr size_t kRrAdaptMinCount = 4096;

// ---- knobs: PGPU_SEQ_DECRYPT, PGPU_PS_DECRYPT, PGPU_RR_ADAPT, PGPU_FIXED_WINDOW, PGPU_WAVE_FORMS (environment at start-up; the
// setters are what pgpu_debug_set_* and the tests use) ----
int seq_policy();            // PGPU_SEQ_DECRYPT: 0 never, 1 by launch size, 2 always, 3 two-lane mode (r03), 4 adaptive (default)
void set_seq_policy(int p);
int ps_policy();             // PGPU_PS_DECRYPT (hensel_ps.hpp): 0 never, 1 by launch size / neighbour lanes (default), 2 always
void set_ps_policy(int p);
int adapt_claim_busy();      // up to how many busy neighbours a part-chip launch claims whole CUs (3; a constant since round 6)
int wave_policy();           // the latency form (hensel_wave.hpp): PGPU_WAVE_FORMS: 0 never, 1 small launches while SIMDs are spare (default), 2 always
void set_wave_policy(int p);
int ps_odd_table();          // PGPU_PS_ODD_TABLE (hensel_ps.hpp): 1 odd-power window table of the one-lane forms (default), 0 half-squared
int set_ps_odd_table(int on);     // returns the previous value
int rr_adapt();              // PGPU_RR_ADAPT: from how many active neighbours on threads on round-robin lanes adapt (3; 0 never)
int set_rr_adapt(int min_busy);   // returns the previous value

// ---- decisions ----
// the by-size part of the sequential-halves policy (modes 3 and 4 decide by size like mode 1, plus their extras)
int seq_policy_by_size();
// with `busy` other batch lanes at work, does a launch of `waves` wavefronts of a part-chip form fill its share of the chip?
bool seq_adaptive(size_t waves, int busy);
// LDS bytes a part-chip launch claims beyond its needs under the adaptive policy (more than half a CU's LDS: one workgroup
// per CU, so that the launches of neighbour lanes spread over the chip); 0: no claim
unsigned adaptive_cu_claim(size_t waves, int busy_lanes);
// CRT decrypt of `count` resident ciphertexts in split form (H, K): the sequential-halves kernel?
bool seq_form_pays(int H, int K, size_t count, int busy = 0);
// ... the one-lane product-scanning kernel of hensel_ps.hpp with K limbs per half (the key must have its constant set)?
// A lone launch runs in ROUNDS of kPsRound ciphertexts (one wavefront per SIMD: 2 x 32768 / 64 = 1024 wavefronts), and a
// round costs the same whether it is full or not -- so the form pays from ps_min_count(K) ciphertexts up, the size from
// which one round beats the multi-lane forms (whose rounds are 16384 / 8192 ciphertexts for 2048- / 3072-bit keys):
// 16385 for 1024- and 2048-bit keys, 24577 for 3072-bit keys ...
constexpr size_t kPsRound = 32768;
size_t ps_min_count(int K);
bool ps_form_pays(size_t count, int busy, int K = 38);
// ... and a lone launch of more than a round whose LAST round would be mostly empty is cut in two: the full rounds take
// this form, the rest a launch of its own in whatever form its size takes (ps_split_head: ciphertexts of the first
// launch; 0: one launch).  65536 + 4464 ciphertexts of a 2048-bit key: 42.7 ms in three rounds, 36 ms as 28 + 8.
size_t ps_split_head(int K, size_t count);
// ... the latency form (hensel_wave.hpp: one exponentiation per wavefront): a lone launch that leaves SIMDs empty even at two
// wavefronts per ciphertext -- up to kSimds / 2 = 512 ciphertexts; not while the one-lane form is forced or switched off
bool wave_form_pays(size_t count, int busy);
// ... and for CT x PT on resident rows (hensel_wave_n2.hpp: one wavefront per ELEMENT): launches of at most one wavefront per SIMD
bool modexp_wave_form_pays(size_t count);
// DJN encrypt onto pair rows / CT x PT / CT + CT of `count` elements in form (H, K): the sequential-halves kernels?
bool fb_encrypt_seq_pays(int H, int K, size_t count, int busy = 0);
bool modexp_seq_form_pays(int H, int K, size_t count);
bool pair_mul_seq_pays(int H, int K, size_t count);
// fixed window of a per-element / secret exponent of exp_bits bits: the w in 1..5 with the fewest products
int pick_window(int exp_bits);
// ... of the CRT-decrypt exponentiation (a secret exponent shared by the launch): w = 6 as well from 1280 bits up
// (entry_bytes: one table entry of every exponentiation of the launch; w = 6 only while the whole table stays under 4 GiB)
// one_lane: the launch runs a one-lane form (hensel_ps.hpp / hensel_ps_bal.hpp) -- the w in 1..6 of the least count of the
// half-squared table weighted by the instructions of a pair squaring and a pair product: 6 from 1024-bit exponents up, same
// cap.  The odd-power table's own counts give the same widths for 512-, 1024- and 1536-bit exponents (policy.cpp)
int pick_decrypt_window(int exp_bits, size_t entry_bytes = 0, bool one_lane = false);
// (pair squarings, pair products) of one exponentiation of a one-lane form at width w
void ps_one_lane_ops(int exp_bits, int w, bool odd, long* squarings, long* products);
// PGPU_FIXED_WINDOW from inside the process (tests): w in 1..6 forces, 0 gives the rules back; returns what was set before
int set_fixed_window(int w);
// ... under the masked table gather (every entry of the table read at every window product: small on purpose)
int masked_decrypt_window();


// ---- the pair form of a key: the ONE rule from the bit length of n to the (G, K) form of its resident pair rows ----
// The form of fewest lanes among those with element-wise kernels (launch.hpp: pair_ops_has) whose radix leaves the lazy
// bounds their room: R = 2^(29 G K) >= 2^8 P for the loop modulus P = n k < 2^(bits + 29), i.e. 29 G K >= bits + 29 + 8.
// The key builders (capi_keys.inc: build_hensel_pub for a public key, pair_l2_for_modulus for a private one) and the plan
// calls (matvec_geometry, pack_geometry) all ask this function; tests/cpp/key_width_policy_tests.cpp sweeps it.
//     bits of n      form     limbs per half (a row is twice that)
//        1 .. 1065   (2,19)    38
//     1066 .. 2051   (4,18)    72    -- also 1066 .. 1123, whose smallest 4-lane modexp form (4,10) has no pair kernels
//     2052 .. 3211   (8,14)   112
//     3212 .. 4139   (8,18)   144    only in builds with PGPU_WITH_4096; else none
//     wider                   none: every resident operation runs on word rows, the aggregation calls refuse
bool pair_form_for_bits(int n_bits, int* G, int* K);
// the form with the same limbs per half on twice the lanes that small launches take beside (G, K) -- (8,9) beside (4,18):
// element-wise operations, DJN encrypt, segment_sum, pack (launch.hpp: pair_ops_alt_has, hensel_fb_encrypt_has,
// segsum_wide_has, pack_wide_has); a key with pair form (G, K) carries its constants too.  false: none compiled
bool pair_wide_form(int G, int K, int* wide_G, int* wide_K);
// every split form of n^2 a public key over an n of n_bits bits builds constants for (capi_keys.inc: build_hensel_pub), in
// the order of its list: per lane count 8, 4, 2 the smallest compiled form (fixed-base or generic modexp kernel) with
// 29 H K >= bits + 29 + 8 -- the forms of one-shot operations on host words, most lanes first --, then the wide form, then
// the pair form LAST: the list's back() is what defines the key's resident rows.  For most widths the last two are what
// the per-lane-count search finds anyway; keys of 1066 .. 1123 bits, whose smallest 4- and 8-lane forms (4,10) and (8,5)
// have no pair kernels, receive (8,9) and (4,18) in addition.  Empty: no split form (word rows everywhere).
void pub_forms_for_bits(int n_bits, std::vector<std::pair<int, int>>* forms);


// ---- the encrypted matrix-vector product (hensel_matvec.hpp; pgpu_batch_ct_matvec, pgpu_ct_matvec_plan) ----
// Y[i] = prod_j X[j]^W[i][j] as an interleaved fixed-window multi-exponentiation: window tables of the cols ciphertexts
// shared by all rows, one group of G lanes per (row, column slice).  Counted in pair products a call costs
//     cols * (2^w - 2)                table build
//   + rows * S * e_bits               squarings (every slice runs its own chain)
//   + rows * cols * ceil(e_bits / w)  multiplications by table entries
//   + rows * (S - 1)                  fold of the partial products.
// Geometry of the key class: its pair form (pair_form_for_bits) where the aggregation kernels are compiled for it
// (launch.hpp: matvec_has -- the sequential-halves forms of hensel_modexp_seq_kernel): (2,19) up to 1065-bit n, (4,18) up
// to 2051, (8,14) up to 3211; false: no pair rows (wider keys), or pair rows without these kernels ((8,18), 4096-bit builds).
bool matvec_geometry(int key_bits, int* G, int* K);
// S: the smallest slice count that puts a wavefront on every SIMD -- a wavefront holds 64/G rows of one slice -- but a
// slice keeps at least kMatvecMinSliceCols columns, so that the e_bits squarings every slice repeats stay at most
// w / (w + kMatvecMinSliceCols) of its products; where the rows alone fill the chip S = 1.  1 <= S <= cols.
// PGPU_MATVEC_SLICES=S forces it (clamped to 1..cols; read at every call: the tests reach every path with it).
constexpr size_t kMatvecMinSliceCols = 4;
size_t matvec_slices(int G, size_t rows, size_t cols);
// w in 1..6 with the fewest products above, among those whose table (cols * 2^w rows of row_bytes) stays under
// kMatvecTableCap -- the Infinity Cache, which the multiply path reads its entries from.  PGPU_MATVEC_WINDOW=w forces it.
constexpr size_t kMatvecTableCap = (size_t)256 << 20;
int matvec_window(size_t rows, size_t cols, int e_bits, size_t slices, size_t row_bytes);
// products of the schedule above (w, S as given)
double matvec_products(size_t rows, size_t cols, int e_bits, int w, size_t slices);


// ---- the encrypted matrix product (hensel_matmul.hpp; pgpu_batch_ct_matmul, pgpu_ct_matmul_plan) ----
// Y[v][i] = prod_j X[v][j]^W[i][j] for n_vec vectors: the matvec above, walked in TILES of `tile` vectors -- one pass
// builds the window tables of its tile*cols ciphertexts, runs one group of G lanes per output (v, i) and column slice, and
// folds the slices; the next pass reuses the table block.  A pass over t vectors costs, in pair products,
//     t * cols * (2^w - 2)                table build
//   + t * rows * S * e_bits               squarings
//   + t * rows * cols * ceil(e_bits / w)  multiplications by table entries
//   + t * rows * (S - 1)                  fold of the partial products,
// with S the matvec's slice rule for the t * rows outputs of the pass (matvec_slices without its knob; the short last
// pass of a call has its own S).  The table and the multiplications sum to the same whatever the tile; the tile decides
// how many outputs a launch has, hence S, and -- the reason it exists -- how large a table one pass holds: under
// kMatvecTableCap at the window the product count wants, however many vectors the call has.
// matmul_plan: w in 1..6 and tile in 1..n_vec with tile * cols * 2^w * row_bytes <= kMatvecTableCap, the pair with the
// fewest products of the whole call (ceil(n_vec / tile) passes, the last one short where tile does not divide n_vec);
// ties go to the larger tile, then to the smaller window.  Where one vector's table at w = 1 exceeds the cap: tile = 1,
// w = 1, as matvec_window leaves such a vector.  n_vec = 1 gives matvec_window and matvec_slices.
// PGPU_MATMUL_WINDOW=w, PGPU_MATMUL_TILE=t, PGPU_MATMUL_SLICES=S force the three values (clamped to 1..6, 1..n_vec,
// 1..cols; a forced S holds for every pass; a forced value is not held against the cap; read at every call: the tests
// reach every path with them).
struct MatmulPlan {
  int window = 1;
  size_t tile = 1;          // vectors of a full pass
  size_t passes = 1;        // ceil(n_vec / tile)
  size_t last = 1;          // vectors of the last pass: n_vec - (passes - 1) * tile, 1 .. tile
  size_t slices = 1;        // S of a full pass
  size_t last_slices = 1;   // S of the last pass (== slices where passes == 1 or last == tile)
  double products = 0;
};
// S of a pass over t vectors under the rule above (forced: PGPU_MATMUL_SLICES)
size_t matmul_slices(int G, size_t t, size_t rows, size_t cols);
// products of the whole call for given w and tile, S by matmul_slices pass by pass
double matmul_products(int G, size_t n_vec, size_t rows, size_t cols, int e_bits, int w, size_t tile);
void matmul_plan(int G, size_t n_vec, size_t rows, size_t cols, int e_bits, size_t row_bytes, MatmulPlan* plan);


// ---- the signed-weight matvec and matmul (hensel_signed.hpp; pgpu_batch_ct_matvec_signed / _matmul_signed and their plans) ----
// The two calls above for weights in two's complement: x^-1 by the batched inversion (invert_products below: 3 (E - 1) for
// E elements, once per call), a table of 2^w + 1 rows per element over [x ; x^-1] (row 0 = one, x^1..x^h, x^-1..x^-h,
// h = 2^(w-1): 2 (h - 1) = 2^w - 2 products, as the unsigned table), and radix-2^w Booth digits of the weights (as many as
// unsigned digits: ceil(e_bits / w)).  So the counts are the unsigned ones plus the inversion; slices and tile rules are the
// unsigned ones, the window minimises the same count, and only the cap sees the longer table:
//     cols * (2^w + 1) * row_bytes <= kMatvecTableCap          (tile * cols * ... for the matmul).
// PGPU_MATVEC_WINDOW / _SLICES and PGPU_MATMUL_WINDOW / _TILE / _SLICES force the signed calls too (read at every call).
int matvec_signed_window(size_t rows, size_t cols, int e_bits, size_t slices, size_t row_bytes);
double matvec_signed_products(size_t rows, size_t cols, int e_bits, int w, size_t slices);
// plan->products includes the inversion of all n_vec * cols elements
void matmul_signed_plan(int G, size_t n_vec, size_t rows, size_t cols, int e_bits, size_t row_bytes, MatmulPlan* plan);


// ---- the encrypted 2-D convolution (hensel_conv.hpp; pgpu_batch_ct_conv2d, pgpu_ct_conv2d_plan) ----
// out[n][co][oy][ox] = prod_{ci,ky,kx} x[n][ci][oy*sh + ky - ph][ox*sw + kx - pw]^w[co][ci][ky][kx] for n_img images: the
// matrix product above with the table of an item apart from the terms of an output.  The tile is whole images per pass.
// With elems = c_in*h*w (the table elements of an image), n_o = c_out*oh*ow (its outputs) and taps = c_in*kh*kw (the terms
// of an output, padded ones counted: they are multiplied by one), a pass over t images costs, in pair products,
//     t * elems * (2^w - 2)               table build
//   + t * n_o * S * e_bits                squarings
//   + t * n_o * taps * ceil(e_bits / w)   multiplications by table entries
//   + t * n_o * (S - 1)                   fold of the partial products,
// with S the matvec's slice rule for t * n_o outputs over taps columns -- carried over as it stands, not fitted to this
// kernel (the short last pass of a call has its own S).
// conv_plan: w in 1..6 and tile in 1..n_img with tile * elems * 2^w * row_bytes <= kMatvecTableCap, the pair with the
// fewest products of the whole call; ties go to the larger tile, then to the smaller window.  Where one image's table at
// w = 1 exceeds the cap: tile = 1, w = 1.  A kernel equal to the image without padding and n_img = 1 gives matvec_window
// and matvec_slices for rows = c_out, cols = elems.
// PGPU_CONV_WINDOW=w, PGPU_CONV_TILE=t, PGPU_CONV_SLICES=S force the three values (clamped to 1..6, 1..n_img, 1..taps; a
// forced S holds for every pass; a forced value is not held against the cap; read at every call).
using ConvPlan = MatmulPlan;   // tile / last: images of a pass
size_t conv_slices(int G, size_t t, size_t n_o, size_t taps);
double conv_products(int G, size_t n_img, size_t elems, size_t n_o, size_t taps, int e_bits, int w, size_t tile);
void conv_plan(int G, size_t n_img, size_t elems, size_t n_o, size_t taps, int e_bits, size_t row_bytes, ConvPlan* plan);
// The signed call (hensel_conv_signed.hpp; pgpu_batch_ct_conv2d_signed, pgpu_ct_conv2d_signed_plan): conv_plan with two
// changes, the relation matmul_signed_plan has to matmul_plan -- the cap is held against the signed table,
//     tile * elems * (2^w + 1) * row_bytes <= kMatvecTableCap,
// and plan->products includes the one inversion of all n_img * elems elements (invert_products).  The per-pass counts, the
// slice rule, the ties and the three knobs are conv_plan's.
void conv_signed_plan(int G, size_t n_img, size_t elems, size_t n_o, size_t taps, int e_bits, size_t row_bytes, ConvPlan* plan);
// the sizes of a shape d = {n_img, c_in, h, w, c_out, kh, kw, stride_h, stride_w, pad_h, pad_w} (the order of
// pgpu_conv2d_shape).  false -- what both C-ABI calls refuse of a shape alone: a dimension or stride equal to 0, pad >=
// kernel, kernel > padded image, an image or kernel side of 2^30 or more, a size product beyond size_t.
struct ConvDims {
  size_t oh, ow, elems, taps, n_o, x_count, w_count, out_count;
};
bool conv_geometry(const size_t d[11], ConvDims* g);


// ---- the encrypted segmented sum (hensel_segsum.hpp; pgpu_batch_ct_segment_sum, pgpu_ct_segment_sum_plan) ----
// out[g][s] = prod_{j : ids[g][j] == s} X[j].  A segment of m elements costs m - 1 pair products however it is cut, so the
// cut decides only how the products spread over the chip and what each chain pays beside them.
// 1. segsum_sort: a stable counting sort of every group's element numbers by id.  perm holds, group after group and
//    segment after segment, the element numbers j in rising order; offsets[g * n_segments + s] .. [.. + 1] is the range of
//    segment s of group g.  Ids equal to kSegsumNone are left out.  false: an id >= n_segments (nothing is written then).
constexpr uint32_t kSegsumNone = 0xFFFFFFFFu;
bool segsum_sort(const uint32_t* ids, size_t groups, size_t cols, size_t n_segments, std::vector<uint32_t>* perm,
                 std::vector<size_t>* offsets);
// 2. the chunk: one chunk is one product chain of one group of G lanes.  The chunk that gives every SIMD
//    kSegsumWavesPerSimd wavefronts -- of 64/G chains each -- to work through at level 0,
//    elements / (kSegsumWavesPerSimd * kSimds * 64/G), but
//    * at least kSegsumMinChunk: a chunk of c entries leaves one partial row (written once, read once by the next level)
//      per c - 1 products, one descriptor for the host to make and upload, and every level is a launch of its own;
//    * at most kSegsumMaxChunk: a chunk is serial, and the wavefronts of a level that are still running when the others
//      are done leave the chip idle for up to one chunk's time.
//    The kernels are fastest with MANY short chains -- two resident wavefronts per SIMD cover each other's row loads, and
//    the queue behind them evens out the tail -- while the host's share of a call grows with the number of chunks; the
//    sweep behind the three constants is in DESIGN.md section 12 and profiles/segsum_bench.txt.
//    PGPU_SEGSUM_CHUNK=c, 2 <= c <= kSegsumForcedMax, forces it (larger values are clamped; read at every call: the
//    tests reach every path with it).
constexpr size_t kSegsumWavesPerSimd = 8;
constexpr size_t kSegsumMinChunk = 8;
constexpr size_t kSegsumMaxChunk = 256;
constexpr size_t kSegsumForcedMax = 65536;
int segsum_chunk(int G, size_t elements);
//    A level whose chains leave SIMDs empty even at 64/wide_G chains per wavefront runs in the form with the same limbs
//    per half on wide_G > G lanes (2048-bit keys: (8,9) beside (4,18); launch.hpp: segsum_wide_has): the same rows, half
//    the serial time per product -- small inputs and the last fold levels cost by their depth, not their size.
bool segsum_wide_pays(int wide_G, size_t chains);
// 3. levels: a segment of more than `chunk` entries leaves ceil(m / chunk) partial rows, which the next level treats as a
//    segment of that length: ceil(log_chunk(longest)) levels, at least 1.
int segsum_levels(int chunk, size_t longest);
// 4. the plan: per level the chunk descriptors, ordered by len descending (stable), and the number of partial rows the
//    level writes.  Level 0 walks perm (begin: an entry of perm), the later ones the partial rows of the level before
//    (begin: a row).  dst: the segment number g * n_segments + s for the last chunk of a segment, else kSegsumPartial | row.
struct SegsumLevel {
  std::vector<SegsumChunk> chunks;
  size_t partial_rows = 0;
};
struct SegsumPlan {
  int chunk = 0;
  size_t longest = 0;
  std::vector<SegsumLevel> levels;    // size() == segsum_levels(chunk, longest)
};
void segsum_plan(const std::vector<size_t>& offsets, int chunk, SegsumPlan* plan);


// ---- the encrypted sparse matrix-vector product (hensel_spmv.hpp; pgpu_batch_ct_spmv, pgpu_ct_spmv_plan) ----
// out[i] = prod_t X[col_idx[t]]^w[t] over the CSR entries t of row i: the window tables of the matvec shared by all rows,
// one group of G lanes per CHAIN of at most `chunk` consecutive CSR entries of one row.  Counted in pair products a row of
// m entries cut into c = max(1, ceil(m / chunk)) chains costs
//     c * e_bits               squarings (every chain runs its own)
//   + m * ceil(e_bits / w)     multiplications by table entries
//   + (c - 1)                  fold of the partial products,
// and the table cols * (2^w - 2) once.  (As in matvec_products the top window's w squarings, which no chain runs, and the
// product the first entry of a chain saves are counted all the same.)
// 1. the chunk: the one that gives every SIMD kSegsumWavesPerSimd wavefronts of 64/G chains, nnz / (that many chains), but
//    * at least kSpmvMinChunk = kMatvecMinSliceCols entries, section 11's reason: the e_bits squarings a chain repeats stay
//      at most w / (w + kSpmvMinChunk) of its products;
//    * at most kSpmvMaxChunk = kSegsumMaxChunk entries: one very long row does not become one serial chain.
//    `rows` bounds nothing yet: a matrix of many short rows has its chains given by the rows, whatever the chunk.
//    All three constants are CARRIED OVER from sections 11 and 12, not fitted to this kernel.  The one sweep of
//    PGPU_SPMV_CHUNK made so far (profiles/spmv_bench.txt: 2^20 non-zeros, 2048-bit key) confirms the
//    fill on 1024 rows of about 1024 entries, finds rows of exactly 16 entries 6 % faster uncut -- here a cut costs e_bits
//    squarings, which the rule does not weigh -- and reaches neither the floor's nor the ceiling's reason.
//    PGPU_SPMV_CHUNK=c, 1 <= c <= kSegsumForcedMax, forces it (larger values are clamped; read at every call: the tests
//    reach every path with it).
constexpr size_t kSpmvMinChunk = kMatvecMinSliceCols;
constexpr size_t kSpmvMaxChunk = kSegsumMaxChunk;
int spmv_chunk(int G, size_t nnz, size_t rows);
// 2. the plan.  chains: level 0, one descriptor per chain -- begin: a CSR position, dst: the output row, or kSegsumPartial |
//    a partial row when the row has several chains; an empty row is a chain of length 0 -- ordered by len descending
//    (stable).  fold: exactly what segsum_plan makes of a segmented sum over those partial rows (rows of one chain appear
//    there as empty segments and are dropped: their result is already written); fold.levels may be empty.
//    The fold runs with the chains' own chunk (at least 2).  false: row_ptr does not start at 0 or decreases, or rows, nnz or
//    the chains reach 2^31, more than the fields of a descriptor address (nothing is written then).
struct SpmvPlan {
  int chunk = 0;
  size_t longest = 0;                 // entries of the longest row
  size_t n_chains = 0;                // == chains.size()
  size_t partial_rows = 0;            // rows the spmv launch writes for the fold levels
  std::vector<SegsumChunk> chains;
  SegsumPlan fold;
};
bool spmv_plan(const uint64_t* row_ptr, size_t rows, int chunk, SpmvPlan* plan);
//    launches of the call without the table build: 1 + fold levels, from the longest row alone
int spmv_levels(int chunk, size_t longest);
// 3. products of the schedule for given totals (chains: over all rows), table included; and the window: w in 1..6 with the
//    fewest products among those whose table (cols * 2^w rows of row_bytes: EVERY column of x, referenced or not) stays
//    under kMatvecTableCap.  PGPU_SPMV_WINDOW=w forces it.
double spmv_products(size_t rows, size_t cols, size_t nnz, size_t chains, int e_bits, int w);
int spmv_window(size_t rows, size_t cols, size_t nnz, size_t chains, int e_bits, size_t row_bytes);
//    the signed call (hensel_spmv_signed.hpp; pgpu_batch_ct_spmv_signed, pgpu_ct_spmv_signed_plan): the same counts plus the
//    inversion of EVERY column of x (invert_products(cols)), the window minimising the unsigned count among those whose
//    table of cols * (2^w + 1) rows stays under the cap.  Chunk, chains and fold are the unsigned call's; PGPU_SPMV_WINDOW /
//    _CHUNK force the signed call too.
double spmv_signed_products(size_t rows, size_t cols, size_t nnz, size_t chains, int e_bits, int w);
int spmv_signed_window(size_t rows, size_t cols, size_t nnz, size_t chains, int e_bits, size_t row_bytes);
//    chains of a matrix of which only rows, nnz and the longest row are known (the plan call): the longest row cut by the
//    chunk, the other rows taken as equally long -- exact while no row is longer than the chunk and for rows of one length,
//    an estimate otherwise
size_t spmv_chains_estimate(size_t rows, size_t nnz, size_t longest, int chunk);


// ---- the encrypted segmented prefix sum (hensel_segscan.hpp; pgpu_batch_ct_segment_scan, pgpu_ct_segment_scan_plan) ----
// out[r][t] = prod_{u <= t} X[r][u] (reverse: u >= t), x read as [rows][seg_len].  One chain of one group of G lanes
// scans a row of m entries with m - 1 products, which is all the work there is; a row longer than the chunk is scanned by
// reduce-then-scan and costs about twice that:
//   up-sweep    the chunks of a row are counted in scan direction (reverse: from the row's end), each of `chunk` entries
//               but the last.  segsum_kernel (perm == null) multiplies every chunk but the last into a total: rows *
//               (nchunks - 1) SegsumChunks of len chunk, total k of row r at row r * (nchunks - 1) + k of the level's
//               totals;
//   recursion   the totals, [rows][nchunks - 1], are scanned FORWARD by the same procedure (they are already numbered in
//               scan direction): the carries;
//   down-sweep  segscan_kernel walks every chunk: chunk 0 of a row starts as its first entry, chunk k > 0 from carry
//               k - 1 of its row, and every running product is stored.
// 1. the chunk: seg_len itself -- one level, one launch, no product more than needed -- when the rows alone give every
//    SIMD kSegscanWavesPerSimd wavefronts of 64/G chains (the fill segsum_chunk aims at), or when seg_len is at most
//    kSegscanMinChunk; otherwise the chunk that makes rows * nchunks reach that fill, at least kSegscanMinChunk (a chunk of
//    c entries leaves a total and a carry row, two descriptors, and every level is two launches).  The figures are
//    segsum_chunk's; the sweep that is to confirm them (tools/bench_segscan.py --sweep) is described in DESIGN.md
//    section 13.  PGPU_SEGSCAN_CHUNK=c, 2 <= c <= kSegscanForcedMax, forces
//    it (larger values are clamped; read at every call).
constexpr size_t kSegscanWavesPerSimd = 8;
constexpr size_t kSegscanMinChunk = 8;
constexpr size_t kSegscanForcedMax = 65536;
int segscan_chunk(int G, size_t rows, size_t seg_len);
// 2. levels: the depth of the hierarchy, 1 for seg_len <= chunk; a call runs 2 * levels - 1 launches (an up-sweep per
//    level but the deepest, then a scan per level).  products: the pair products of all of them, padding excluded:
//    rows * (seg_len - 1) for one level, else rows * ((seg_len - 1) + (nchunks - 1) * (chunk - 1)) plus the recursion's.
int segscan_levels(int chunk, size_t seg_len);
size_t segscan_products(int chunk, size_t rows, size_t seg_len);
//    false: the totals of level 0 -- the most any level has -- are more rows than a descriptor's 31-bit total / 32-bit carry
//    field names, or rows * seg_len overflows
bool segscan_fits(int chunk, size_t rows, size_t seg_len);
// 3. the plan: levels[0] reads x and writes the result; levels[l] reads the totals of level l - 1 and writes its carries.
//    Execution order: up of level 0, 1, ..., then scan of the deepest level, ..., 1, 0.  scan is ordered by len descending
//    (only the last chunk of a row is shorter).  begin: the first row of the level's input the chain touches (reverse: the
//    highest); carry: a row of what level l + 1 wrote, or kSegscanNoCarry.
struct SegscanLevel {
  size_t rows = 0, seg_len = 0;       // the level's input (and output) as [rows][seg_len]
  bool reverse = false;
  std::vector<SegsumChunk> up;        // empty in the deepest level
  size_t totals = 0;                  // rows the up-sweep writes = rows * seg_len of the next level
  std::vector<SegscanChunk> scan;
};
struct SegscanPlan {
  int chunk = 0;
  size_t products = 0;                // == segscan_products(chunk, rows, seg_len)
  std::vector<SegscanLevel> levels;   // size() == segscan_levels(chunk, seg_len)
};
void segscan_plan(size_t rows, size_t seg_len, int chunk, bool reverse, SegscanPlan* plan);


// ---- the batched inversion (hensel_invert.hpp; pgpu_batch_ct_negate / _sub, pgpu_ct_negate_plan) ----
// out[i] = x[i]^-1 mod n^2 by simultaneous inversion.  The batch is cut into chains of at most `chunk` consecutive rows;
//   forward    segscan_kernel (no carries) stores the running products of every chain: count - chains products;
//   recursion  the chain totals -- ceil(count / chunk) rows -- are inverted by the same procedure; a level of at most chunk
//              rows is ONE chain, whose total the host inverts (one row down, one modular inversion, one row up);
//   walk back  invert_walk_kernel walks every chain from the inverse of its total: 2 (len - 1) products per chain.
// A level of m rows in k chains costs 3 (m - k) products and leaves k rows to the next one; the top level has one chain:
// 3 (count - 1) products in all, whatever the chunk.  The chunk only trades chains in flight against levels (two launches
// each, and the top chain is serial).
// 1. the chunk of a level of m rows: the one that gives every SIMD kSegscanWavesPerSimd wavefronts of 64/G chains (the fill
//    segscan_chunk aims at), m / (that many chains), at least kInvertMinChunk.  The rule is applied level by level, so a
//    batch that fills the chip is cut into chains that just fill it, and every level that cannot fill it anyway -- all the
//    levels above, and small batches -- is cut into pairs: there a level costs by the depth of its chains, 3 (chunk - 1)
//    serial products, and the depth of the whole hierarchy, 3 (chunk - 1) log_chunk(count), is least at 2 (measured,
//    tools/bench_negate.py --sweep, DESIGN.md section 22: the floor of 8 carried over from segscan_chunk took 1.5 to 1.9
//    times the kernel time at 64 to 65536 elements).  The fill figure itself is carried over and was not swept.
//    PGPU_INVERT_CHUNK=c, 2 <= c <= kInvertForcedMax, forces c at every level (larger values are clamped; read at every call).
constexpr size_t kInvertMinChunk = 2;
constexpr size_t kInvertForcedMax = kSegscanForcedMax;
int invert_chunk(int G, size_t m);
// 2. levels: the depth of the hierarchy -- a level of at most its chunk rows is the top.  launches: a forward pass and a
//    walk back per level, what the timing record shows for pair-row input; count == 1 has nothing to multiply forward and
//    is one walk back.  products: 3 (count - 1), padding excluded.
int invert_levels(int G, size_t count);
int invert_launches(int G, size_t count);
size_t invert_products(size_t count);
//    false: level 0 has more chains than the 32-bit carry field of a descriptor names, or 3 * count overflows
bool invert_fits(int G, size_t count);
// 3. the form of a level: the wide one (launch.hpp: invert_wide_has; 2048-bit keys: (8,9) beside (4,18)) when even 64 /
//    wide_G chains per wavefront put at most one wavefront on a SIMD -- segsum_wide_pays' rule, carried over; measured
//    (section 22): the wide form takes 0.71-0.75 of the base form's time at 64 to 65536 elements.
//    PGPU_INVERT_WIDE=0 / 1 forces the base / the wide form where the key has one (read at every call).
bool invert_wide_pays(int wide_G, size_t chains);
// 4. the plan: levels[0] reads x and writes the result; levels[l] reads the totals of level l - 1 -- the last running
//    product of each of its chains, in chain order -- and writes their inverses.  Execution order: forward of level 0, 1,
//    ..., the host inversion of the top chain's total, then the walk back of the top level, ..., 1, 0.  Chain j of a level
//    covers the rows j * chunk ... of it (only the last chain is shorter: the lists are ordered by len descending as they
//    stand).  fwd: carry == kSegscanNoCarry; back: the same chains with carry = j, the row of the level above's output
//    (top level: row 0 of the uploaded inverse).
struct InvertLevel {
  size_t n = 0;                       // rows of the level's input (and output)
  int chunk = 0;                      // == invert_chunk(G, n)
  std::vector<SegscanChunk> fwd, back;
};
struct InvertPlan {
  int chunk = 0;                      // of level 0
  size_t products = 0;                // == invert_products(count)
  std::vector<InvertLevel> levels;    // size() == invert_levels(G, count)
};
void invert_plan(size_t count, int G, InvertPlan* plan);

// ---- the encrypted slot packing (hensel_pack.hpp; pgpu_batch_ct_pack, pgpu_ct_pack_plan) ----
// One Horner chain of (seg_len - 1) * (slot_bits + 1) products per output row, one launch, every chain equally long: there
// is no plan but the form.  The rows are few by construction (count / seg_len), and a launch whose wavefronts leave SIMDs
// empty costs by the depth of one chain: such a launch runs in the form with the same limbs per half on wide_G > G lanes
// (2048-bit keys: (8,9) beside (4,18); launch.hpp: pack_wide_has) -- the same rows, half the serial time per product --
// when even 64 / wide_G chains per wavefront put at most one wavefront on a SIMD (segsum_wide_pays' rule: up to 8192 rows).
// The rule is carried over from the segmented sum; measured: the wide form takes 0.80 of the base
// form's time at 64 and 2048 rows, 0.82 at 8192, 1.33 at 16384 and 1.29 at 32768; nothing was measured between 8192
// and 16384 rows, so the switch at 8192 is on the right side of both neighbours and not located more finely.
// PGPU_PACK_WIDE=0 / 1 forces the base / the wide form where the key has one (read at every call: the measurement).
bool pack_wide_pays(int wide_G, size_t rows);
// the (G, K) form a call over `rows` output rows launches for keys of key_bits; false: no pair rows for such keys
bool pack_geometry(int key_bits, size_t rows, int* G, int* K);


// ---- the encrypted weighted sum of K resident batches (hensel_wsum.hpp; pgpu_batch_ct_weighted_sum,
//      pgpu_ct_weighted_sum_plan) ----
// out[i] = prod_k X_k[i]^(a_k), one plaintext weight per BATCH: the weights are the same for every element, so the
// schedule is built here, once, and is uniform for the launch.
// 1. the schedule of one slice of the terms: from the highest set bit over the slice's weights down to bit 0 one SQR step
//    per bit (none before the top bit), after it one MUL k step for every term k of the slice whose weight has that bit
//    set, in term order.  The accumulator is LOADED from the first operand (WsumSlice::first), not multiplied into a one:
//    a slice whose weights are L bits long costs (L - 1) squarings and (sum of popcounts - 1) general products, and its
//    step list holds exactly that many steps.  A zero weight contributes nothing and its batch is never named.
// 2. the slices: the terms are cut into S contiguous ranges of floor/ceil(n_terms / S) terms; every slice runs its own
//    squarings, the partial rows are folded afterwards (one product per further slice).  S is the matvec's rule, CARRIED
//    OVER from section 11, not fitted to this kernel: the smallest S that puts a wavefront on every SIMD for this count
//    and G, while a slice keeps at least kMatvecMinSliceCols terms (the squarings a slice repeats stay a bounded share of
//    its products); 1 <= S <= n_terms.  Without weights (all ones) there are no squarings and a cut costs one fold product
//    only: the cap is then "at least 2 terms per slice".  Slices whose weights are all zero are dropped; when every
//    weight is zero one slice remains whose `first` is kWsumNone (the ciphertext 1, no product).
//    PGPU_WSUM_SLICES=s forces S (clamped to n_terms; read at every call: the tests reach every path with it).
constexpr size_t kWsumMaxTerms = 65535;
size_t wsum_slices(int G, size_t count, size_t n_terms, bool unit_weights);
// 3. the form: (2,19), (4,18), (8,14) by pair_form_for_bits; a 2048-bit key has the (8,9) form beside (4,18) -- the same
//    rows, half the serial time per product, half the chains per wavefront -- for launches of `chains` = count * slices
//    chains that put at most one wavefront on a SIMD even then (segsum_wide_pays' rule, as pack_wide_pays carries it).
//    PGPU_WSUM_WIDE=0 / 1 forces the base / the wide form (read at every call).
bool wsum_wide_pays(int wide_G, size_t chains);
bool wsum_geometry(int key_bits, size_t chains, int* G, int* K);
// 4. the plan.  weights: [n_terms][w_words] little-endian 64-bit words, or null: every weight is 1.  slices: only the
//    non-empty ones (dst unset: the call fills it in), steps: their lists one after the other.  products is per ELEMENT:
//    the steps of all slices plus (slices - 1) for the fold -- exact, the idle groups of a last wavefront not counted.
//    false: n_terms == 0 or beyond kWsumMaxTerms, S == 0, w_words < 1 with weights, or a slice of 2^31 steps or more
//    (nothing is written then).
struct WsumPlan {
  std::vector<WsumSlice> slices;      // >= 1 entry
  std::vector<WsumStep> steps;
  size_t longest = 0;                 // steps of the longest slice
  size_t squarings = 0, muls = 0;     // over all slices, the fold not included
  size_t products = 0;                // squarings + muls + (slices.size() - 1)
  bool all_zero = false;              // every weight is zero: one slice, first == kWsumNone
};
bool wsum_plan(const uint64_t* weights, int w_words, size_t n_terms, size_t S, WsumPlan* plan);


// ---- the bucket-method encrypted matvec (hensel_bucket.hpp; pgpu_batch_ct_matvec_bucket, pgpu_ct_matvec_bucket_plan) ----
// Y[i] = prod_j X[j]^W[i][j] without window tables: every weight is cut into W = ceil(e_bits / c) digits of c bits, and
// per (row, window)
//   accumulate   the columns whose digit is d >= 1 are multiplied into bucket B_d: a segmented sum over rows * W groups
//                of 2^c segments (bucket 0 and every empty bucket: the row of one), the levels of segsum_plan
//   reduce 1     per block k of b buckets (b a power of two, nb = 2^c / b):  U_k = prod_i B[k b + i],
//                V_k = prod_i B[k b + i]^i, by two running products                        (b == 1: skipped, U = B)
//   reduce 2     S = prod_k V_k * (prod_k U_k^k)^b = prod_d B_d^d: the same two running products over the U_k, log2 b
//                squarings, nb products by the V_k                                          (nb == 1: skipped, S = V_0)
//   Horner       out[i] = prod_t S[i][t]^(2^(c t)): pack_kernel over [rows][W] with slot_bits = c (W == 1: no launch)
// Counted in pair products, data-independent upper bounds (a chain that starts from its first entry instead of a one
// saves a product or two of them):
//     rows * W * cols                          accumulate
//   + rows * W * nb * 2 (b - 1)                reduce 1
//   + rows * W * (2 (nb - 1) + log2 b + nb)    reduce 2
//   + rows * (W - 1) * (c + 1)                 Horner
// and in depth -- the products of the call that run one after the other: the longest chain of every accumulation level
// for a bucket that holds every column (chunk = segsum_chunk(G, rows * W * cols): min(chunk, m) at a level of m entries,
// m -> ceil(m / chunk)), 2 (b - 1), 2 (nb - 1) + log2 b + nb, (W - 1) (c + 1).
// bucket_plan: c in 1..kBucketMaxWindow, b = 2^ceil(c / 2); among the c whose bucket block rows * W * 2^c * row_bytes
// stays under kMatvecTableCap (none: c = 1) the one that minimises  products / C + kBucketDepthWeight * depth,  with
// C = kSimds * 2 wavefronts * 64 / G chains at work at a time; ties go to the smaller c.  The depth term is there
// because the product count alone does not see serial reductions: at 2^20 columns of 32 bits c = 8, 9 and 10 are within
// 0.15 % of each other in products (the same W), and c = 10 runs 87 serial products more than c = 8: 8.1 against 6.9 ms.
// PGPU_BUCKET_WINDOW=c and PGPU_BUCKET_BLOCK=b force the two values (clamped to 1..kBucketMaxWindow and 1..2^c, a forced b
// rounded down to a power of two; a forced value is not held against the cap; read at every call: the tests reach every
// path with them).
constexpr int kBucketMaxWindow = 10;
// what the call refuses whatever chose the window: a bucket block beyond this many bytes (7.4 M buckets of a 2048-bit key)
constexpr size_t kBucketBlockMax = (size_t)4 << 30;
// kBucketDepthWeight, from the sweep of tools/bench_bucket.py --sweep (one MI355X, 2048-bit key, forced c = 4..10 at the
// default block; profiles/bucket_bench.txt).  Kernel ms at 1 x 2^20 x 32 / 16 x 65536 x 32:
//     c        4      5      6      7      8      9      10
//     ms   11.51  10.89   9.58   8.51   6.98   7.73   8.20   /   11.16  10.04   8.95   8.07   6.67   7.44   7.87
// A least-squares fit  ms = alpha * products + beta * depth + gamma  gives alpha = 1.04 / 1.07 ns, beta = 9.2 / 11.8 us:
// beta / (alpha * C) = 0.27 / 0.34.  With 0.3 the cost orders all seven windows as measured at both shapes
// (8 < 9 < 10 < 7 < 6 < 5 < 4); the first guess, 1, picked the same winner but put 7 ahead of 9 and 10.  Fitted on these
// two shapes only.
constexpr double kBucketDepthWeight = 0.3;
struct BucketPlan {
  int window = 1;           // c
  int block = 1;            // b
  size_t windows = 1;       // W = ceil(e_bits / c)
  size_t nb = 2;            // 2^c / b
  size_t bucket_bytes = 0;  // rows * W * 2^c * row_bytes
  double products = 0;
  size_t depth = 0;
};
int bucket_default_block(int c);
int bucket_log2(size_t v);      // floor(log2 v), v >= 1
double bucket_products(size_t rows, size_t cols, int e_bits, int c, int b);
size_t bucket_depth(int G, size_t rows, size_t cols, int e_bits, int c, int b);
// (depth_weight: the rule with another weight -- the tests construct exact ties at 0; at 0.3, no binary fraction, a tie is a matter of rounding)
void bucket_plan(int G, size_t rows, size_t cols, int e_bits, size_t row_bytes, BucketPlan* plan,
                 double depth_weight = kBucketDepthWeight);
// the accumulation's sort, digit-aware: what segsum_sort makes of ids[(i * W + t) * cols + j] = digit t of w[i * cols + j]
// (zero: kSegsumNone) over rows * W groups of 2^c segments, without materialising the ids -- a stable counting sort.
// w: [rows * cols][w_words] little-endian 64-bit words; bits at and above e_bits are ignored.
void bucket_sort(const uint64_t* w, int w_words, size_t rows, size_t cols, int e_bits, int c, std::vector<uint32_t>* perm,
                 std::vector<size_t>* offsets);


// ---- plan images: what an aggregation call uploads in one copy (capi_aggregate.inc) ----
// Sections one after the other; add() pads with zero bytes up to a multiple of `align` first and returns the byte offset
// of the section.  src == null leaves the n bytes zero.
struct PlanImage {
  std::vector<char> bytes;
  size_t add(const void* src, size_t n, size_t align = 1);
  template <class T>
  size_t add(const std::vector<T>& v, size_t align = 1) { return add(v.data(), v.size() * sizeof(T), align); }
  const char* data() const { return bytes.data(); }
  size_t size() const { return bytes.size(); }
};
// The images of the four planned calls, and the rows of device scratch their levels rotate through.  Only the leading
// index lists (perm, col_idx) are padded, to 16 bytes, so that the 16-byte descriptors behind them stay aligned; every
// other section is packed.
//   segment sum   perm (never empty: one zero entry stands in, the kernel reads entry 0 for the groups past their end),
//                 then the descriptors of every level, at level_at[l].  Partial rows: level l reads what level l - 1
//                 wrote, so two regions serve all levels in turn -- level l writes region l & 1 of region[l & 1] rows
struct SegsumImage {
  PlanImage image;
  std::vector<size_t> level_at;
  size_t region[2] = {0, 0};
};
void segsum_image(const std::vector<uint32_t>& perm, const SegsumPlan& plan, SegsumImage* out);
//   spmv          col_idx, the chain descriptors at chains_at, the descriptors of every fold level at fold_at[f].  The
//                 chains write region 0, fold level f reads region f & 1 and writes the other one
struct SpmvImage {
  PlanImage image;
  size_t chains_at = 0;
  std::vector<size_t> fold_at;
  size_t region[2] = {0, 0};
};
void spmv_image(const uint32_t* col_idx, size_t nnz, const SpmvPlan& plan, SpmvImage* out);
//   segment scan  per level the up-sweep descriptors at up_at[l], then the scan descriptors at scan_at[l].  Scratch rows:
//                 per level its totals at row totals_at[l] and, beside them, the carries the level below makes of them at
//                 carry_at[l] (the deepest level has neither)
struct SegscanImage {
  PlanImage image;
  std::vector<size_t> up_at, scan_at, totals_at, carry_at;
  size_t scratch_rows = 0;
};
void segscan_image(const SegscanPlan& plan, SegscanImage* out);
//   inversion     per level the forward descriptors at fwd_at[l], then the walk-back descriptors at back_at[l].  Scratch
//                 rows: per level above the first its input (the totals of the level below, gathered) at in_at[l] and its
//                 running products / inverses at out_at[l]  (in_at[0], out_at[0]: unused, x and the result batch)
struct InvertImage {
  PlanImage image;
  std::vector<size_t> fwd_at, back_at, in_at, out_at;
  size_t scratch_rows = 0;
};
void invert_image(const InvertPlan& plan, InvertImage* out);
//   weighted sum  the row bases of the terms (tab), of the slices' results (ftab: empty without a fold), the slice
//                 descriptors of the launch and of the fold, then their step lists
struct WsumImage {
  PlanImage image;
  size_t tab_at = 0, ftab_at = 0, slices_at = 0, fold_slices_at = 0, steps_at = 0, fold_steps_at = 0;
};
void wsum_image(const std::vector<const uint32_t*>& tab, const std::vector<const uint32_t*>& ftab, const WsumPlan& plan,
                const WsumPlan& fold, WsumImage* out);


// ---- gather, concat and slice of resident batches (gather.hpp; pgpu_batch_gather / _concat / _slice,
//      pgpu_batch_gather_plan) ----
// Rows move as bytes.  1. the launch shape, from the row size alone: pieces of 16 bytes where row_bytes % 16 == 0, of 8
//    otherwise; a row is swept by the smallest power of two of lanes that covers its pieces, at most kGatherMaxLanes = 16
//    -- so a wavefront holds 64 / lanes >= 4 rows, each lane up to kGatherUnroll loads ahead of its stores: the recipe
//    measured for gathered whole rows (4 rows in flight per wavefront), never one lane per multi-piece row.  Rows of 8
//    bytes are one piece: one lane each, 64 neighbouring outputs per wavefront.
//    false: row_bytes == 0 or no multiple of 8, or n_out == 0 (nothing is written then).
constexpr uint64_t kGatherOne = ~(uint64_t)0;       // index sentinel: the row of one
constexpr size_t kGatherMaxSources = 65535;
constexpr size_t kGatherMaxRows = 0xFFFFFFFFull;    // a source holds FEWER rows than this (row numbers are 32 bits, all ones is the sentinel)
// the first source that holds kGatherMaxRows rows or more (the call is refused then), or n_src: every count is addressable
size_t gather_counts_ok(const size_t* counts, size_t n_src);
struct GatherPlan {
  int vec_bytes = 0, lanes_per_row = 0, rows_per_wavefront = 0, lanes_log2 = 0;
  size_t wavefronts = 0, blocks = 0;
};
bool gather_plan(size_t row_bytes, size_t n_out, GatherPlan* plan);
// 2. the descriptors: flat index i of the concatenation of sources of counts[0..n_src) rows -> (source, row); kGatherOne ->
//    (0, kGatherOneRow).  A handle named twice is two sources to this function.  Returns n_out, or the FIRST position whose
//    index is at or beyond the total count and not the sentinel (desc is unspecified then).
size_t gather_descs(const size_t* counts, size_t n_src, const uint64_t* idx, size_t n_out, std::vector<GatherDesc>* desc);
//    ... and of the strided slice: rows start, start + step, ... of source 0
void gather_slice_descs(size_t start, size_t count, size_t step, std::vector<GatherDesc>* desc);
// 3. the image: the source bases (8-byte entries), the row of one at a 16-byte boundary, the descriptors
struct GatherImage {
  PlanImage image;
  size_t bases_at = 0, one_at = 0, desc_at = 0;
};
void gather_image(const std::vector<const char*>& bases, const void* one, size_t row_bytes, const std::vector<GatherDesc>& desc,
                  GatherImage* out);

}  // namespace policy
}  // namespace pgpu

#endif  // PAILLIERCRYPTOLIB_AMD_CSRC_POLICY_HPP_
