/* pgpu.h -- C-ABI of the MI355X (gfx950) batched modular-exponentiation engine.
 *
 * This is the drop-in boundary under the reference's `ipcl::` C++ API: every entry point takes
 * plain pointers and sizes (no C++ types, no torch types) and replaces one call the reference
 * makes into a third-party/accelerator primitive.  The precedent in the reference is its own
 * accelerator seam, the HE-QAT C library (module/heqat/heqat/include/heqat/bnops.h:63-148,
 * context.h:18-26) and the IPP-Crypto multi-buffer primitive mbx_exp_mb8 (call site
 * ipcl/mod_exp.cpp:508-516).
 *
 * DATA LAYOUT.  A big integer is `words` little-endian 64-bit limbs (same as the `int64u`
 * arrays handed to mbx_exp_mb8, mod_exp.cpp:486-506).  A batch is row-major
 * [element][limb] with a fixed element stride given in 64-bit words; a stride of 0 means
 * "one shared value for the whole batch" (every reference call site passes N copies of one
 * modulus / one exponent / one base: pub_key.cpp:53-54,67-69, pri_key.cpp:119-120,
 * ciphertext.cpp:151).  Values are zero padded to the stride.
 *
 * OWNERSHIP / THREADING.  The caller owns every buffer it passes.  Functions without the
 * `_dev` suffix take HOST pointers and are synchronous (like release_bnModExp_buffer,
 * bnops.h:134-148): on return the outputs are complete.  `_dev` functions take DEVICE
 * pointers plus a hipStream_t (as void*) and only enqueue work on that stream; calls on different
 * streams never share scratch memory (window tables and the CRT hand-over buffer are per stream), so
 * they may be issued concurrently.  All entry points may be called from several host threads (the
 * reference's APPLEVEL_OMP test calls encrypt/decrypt from 4 threads,
 * test/test_cryptography.cpp:45-57): host-pointer calls run as tasks on the worker lanes of the
 * device pool (two per GPU), so one caller's copies overlap another caller's kernels.
 *
 * DEVICE POOL.  pgpu_init binds the process to one GPU; pgpu_init_all builds a pool over several
 * (the counterpart of acquire_qat_devices taking every QAT instance, heqat/context.h:18-26, and
 * of the reference's own two-way batch split over a second std::thread, mod_exp.cpp:700-731).
 * With a pool, every host-pointer entry point cuts its batch [0, count) into contiguous shards,
 * one per GPU (output order is preserved by construction), and key objects hold one copy of their
 * constants per GPU: the image is uploaded to GPU 0 and reaches the others through one RCCL
 * broadcast over xGMI (per-device copies when RCCL is unavailable).  There is no other collective
 * on the data path.  The `_dev` functions and pgpu_dev_alloc/free/copy address ONE pool entry: the
 * calling thread's current one (pgpu_set_device, default 0).  pgpu_batch handles are the sharded,
 * device-resident form of a batch.
 *
 * SIDE CHANNELS.  Operation sequences do not depend on secret data unless the caller opts in:
 * exponents that are private-key constants (p-1, q-1) run a fixed-window schedule (always w
 * squarings and one multiplication, also for zero digits), the same instruction stream for every
 * key; pgpu_set_secret_exponent_policy(PGPU_EXP_SLIDING) trades that for ~5 % fewer
 * multiplications with a key-dependent schedule.  Table ADDRESSES are not hidden: the window table
 * of a wavefront is indexed by exponent digits (per-key constant pattern for p-1/q-1, per-element
 * for the randomness r of the DJN fixed-base product and for CT*PT exponents), i.e. the engine
 * is not hardened against a co-resident observer of the memory system -- unless
 * pgpu_set_table_gather_policy(1) is chosen, which makes the split-form kernels read every entry of
 * a window table and select; since round 4 that covers the DJN fixed-base product as well (a table of its own
 * with a 4-bit window: 256 products of 16 candidates each instead of 85 indexed ones).
 * Under the default indexed policy the one-lane CRT-decrypt kernels keep only the odd powers of the base
 * in the window table (PGPU_PS_ODD_TABLE, default 1): the table address already follows each digit of
 * p-1 / q-1, and the POSITION of the multiplication inside a window then follows the digit's trailing
 * zeros -- a subset of what the address shows.  Every window still runs w squarings and one
 * multiplication, also for zero digits, so the duration does not depend on the key.  Under
 * pgpu_set_table_gather_policy(1) those kernels keep the full table and the fixed order (w squarings,
 * then the multiplication): a digit-independent instruction order.  Sliding windows stay opt-in.
 * pgpu_batch_gather / _concat / _slice are NOT refused under the masked policy: the address stream depends on the
 * caller's plaintext indices only, as for upload and download.
 * Device copies of private-key constants are zeroed before they are freed.
 *
 * ERRORS.  Every function returns PGPU_OK (0) or a negative pgpu_status; nothing calls
 * exit().  pgpu_last_error() returns a thread-local description.  The C++ layer turns a
 * non-zero status into the reference's ERROR_CHECK exception (utils/util.hpp:23-34).
 * There is NO CPU fallback anywhere behind this interface: without a usable gfx950 device
 * every compute entry point fails with PGPU_ERR_NO_DEVICE.
 */
#ifndef PGPU_H_
#define PGPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pgpu_status {
  PGPU_OK = 0,
  PGPU_ERR_INVALID_PARAM = -1, /* null pointer, zero width, inconsistent sizes            */
  PGPU_ERR_EVEN_MODULUS = -2,  /* Montgomery arithmetic needs an odd modulus               */
  PGPU_ERR_UNSUPPORTED = -3,   /* operand width beyond the compiled kernel geometries      */
  PGPU_ERR_NO_DEVICE = -4,     /* no HIP device / not initialised                          */
  PGPU_ERR_HIP = -5,           /* a HIP runtime call failed (see pgpu_last_error)          */
  PGPU_ERR_NOT_INVERTIBLE = -6 /* key material is inconsistent (e.g. p == q); negate / sub of a non-unit */
} pgpu_status;

/* ---- context: behind ipcl::initializeContext / terminateContext (utils/context.cpp:40-71);
 *      replaces acquire_qat_devices / release_qat_devices (heqat/context.h:18-26) ---- */
int pgpu_init(int device /* HIP ordinal; -1 = keep the current device */);
/* Pool over the first n visible GPUs (0 = all).  With the environment variable
 * PGPU_POOL_OVERSUBSCRIBE=1, n may exceed the number of visible GPUs: pool entries then wrap around
 * the physical devices (validation of the multi-device paths on a single-GPU box). */
int pgpu_init_all(int n_devices_or_0);
void pgpu_shutdown(void);
int pgpu_device_count(void);       /* visible HIP devices */
int pgpu_is_initialized(void);
const char* pgpu_last_error(void);
const char* pgpu_device_name(void); /* of the calling thread's current pool entry */
/* What this library binary was built with (host-side query, needs no device): bit 0 = the split forms of the 4096-bit
 * key class (build switch PGPU_BUILD_4096=1; without them such keys run the full-width kernels).  Results never depend
 * on it.  (Bit 1 named the A/B-wavefront decrypt experiment of rounds 3-5; retired, always 0.) */
#define PGPU_FEATURE_4096_SPLIT 1
int pgpu_build_features(void);
int pgpu_pool_size(void);           /* entries of the pool (0 before init) */
int pgpu_set_device(int pool_index);/* pool entry addressed by this thread's `_dev` / dev_alloc / copy calls */
int pgpu_get_device(void);
/* "rccl" | "memcpy" | "single": how key images reached the pool devices (xGMI broadcast, per-device
 * copies, or a pool of one) */
const char* pgpu_pool_transport(void);
/* why RCCL is (not) in use ("ok", "pool entries share a physical device", the failing call, ...) */
const char* pgpu_rccl_note(void);
/* Replicated key images are read back from every GPU once per upload and compared with the host bytes; a copy
 * that differs is rewritten over PCIe, counted here, and RCCL is retired if it delivered it. */
int pgpu_replication_stats(uint64_t* images_verified, uint64_t* copies_repaired);
/* test hook: flips one byte of the NEXT replicated image on pool entry `pool_index` right after the broadcast */
int pgpu_debug_corrupt_next_replica(int pool_index);
/* batches smaller than min_shard * k elements are spread over at most k GPUs (default 256; env
 * PGPU_MIN_SHARD) */
int pgpu_set_min_shard(size_t min_elements_per_device);
/* waits for everything queued on the pool's own streams (resident-batch operations, worker lanes) on every GPU */
int pgpu_synchronize(void);
/* The cut a batch of `count` elements receives on a pool of `pool_size` GPUs: *n_shards shards, shard i =
 * elements [bounds[i], bounds[i+1]) on pool entry i (contiguous, in order, sizes differ by at most one;
 * bounds has room for pool_size + 1 entries).  Pure host-side query (needs no device): this is the rule every
 * host-pointer entry point and every pgpu_batch follows. */
int pgpu_shard_plan(size_t count, int pool_size, int* n_shards, size_t* bounds);

/* ---- generic batched modular exponentiation: out[i] = base[i]^exp[i] mod mod ----
 * Replaces mbx_exp_mb8 (mod_exp.cpp:508-516) / ippsMontExp (mod_exp.cpp:549-579) under
 * ipcl::modExp (mod_exp.hpp:72-83).  `exp_bits` is the maximum exponent bit length of the
 * batch (the reference computes the same maximum, mod_exp.cpp:484); exponent words above
 * exp_bits must be zero.  The modulus is shared and odd; bases may be any value that fits
 * mod_words words (they are reduced).  out has stride mod_words.
 * A modulus that is the square of an odd root of up to 3072 bits -- every modulus of the Paillier path: n^2, p^2,
 * q^2 -- is recognised (once per modulus) and runs the split form (PGPU_HENSEL=0: never). */
int pgpu_modexp(const uint64_t* base, size_t base_stride, const uint64_t* exp, size_t exp_stride,
                int exp_words, int exp_bits, const uint64_t* mod, int mod_words, uint64_t* out,
                size_t count);
int pgpu_modexp_dev(const uint64_t* d_base, size_t base_stride, const uint64_t* d_exp,
                    size_t exp_stride, int exp_words, int exp_bits, const uint64_t* h_mod,
                    int mod_words, uint64_t* d_out, size_t count, void* hip_stream);

/* ---- batched modular multiplication: out[i] = a[i]*b[i] mod mod ----
 * Replaces the per-element `a * b % sq` of CipherText::raw_add (ciphertext.cpp:135-141);
 * b_stride == 0 is the reference's vector (+) scalar case (ciphertext.cpp:51-58). */
int pgpu_modmul(const uint64_t* a, const uint64_t* b, size_t b_stride, const uint64_t* mod,
                int mod_words, uint64_t* out, size_t count);
int pgpu_modmul_dev(const uint64_t* d_a, const uint64_t* d_b, size_t b_stride,
                    const uint64_t* h_mod, int mod_words, uint64_t* d_out, size_t count,
                    void* hip_stream);


/* ---- Paillier public key: fused encrypt ----
 * Replaces PublicKey::raw_encrypt + applyObfuscator (pub_key.cpp:82-110) for make_secure=true:
 *   DJN key (hs != NULL):  c[i] = hs^r[i]      * (1 + n*m[i]) mod n^2   (pub_key.cpp:51-64)
 *   plain   (hs == NULL):  c[i] = r[i]^n       * (1 + n*m[i]) mod n^2   (pub_key.cpp:66-80)
 * n has n_words words (key bits / 64); hs and c have 2*n_words words.  r is the caller's
 * randomness (the reference draws it on the host too, pub_key.cpp:59-61,74-76, or injects it
 * with setRandom, pub_key.cpp:92-95); it is used as given: not reduced, not truncated. */
typedef struct pgpu_pubkey pgpu_pubkey;
int pgpu_pubkey_create(const uint64_t* n, int n_words, const uint64_t* hs_or_null,
                       pgpu_pubkey** out);
void pgpu_pubkey_destroy(pgpu_pubkey* key);
int pgpu_paillier_encrypt(const pgpu_pubkey* key, const uint64_t* m, size_t m_stride, int m_words,
                          const uint64_t* r, size_t r_stride, int r_words, int r_bits,
                          uint64_t* c, size_t count);
int pgpu_paillier_encrypt_dev(const pgpu_pubkey* key, const uint64_t* d_m, size_t m_stride,
                              int m_words, const uint64_t* d_r, size_t r_stride, int r_words,
                              int r_bits, uint64_t* d_c, size_t count, void* hip_stream);

/* DJN keys: hs is a key constant, so hs^r runs as a fixed-base product over a per-key table of
 * hs^(d*2^(w*i)) (built on the GPU at the first encrypt, no squarings afterwards).  w = 0 selects
 * the generic square-and-multiply kernel instead; default 13 (env PGPU_FB_WINDOW, 0..14): 79 table products
 * for a 1024-bit r, 373 MB of table per 2048-bit key and GPU, built in 73 ms (w = 12: 86 products, 203 MB, 40 ms -- the
 * default until round 4; w = 10: 103 products, 61 MB; encrypt launch of the bench batch 0.775 / 0.835 / 1.19 ms).  The
 * table budgets (pgpu_set_fixed_base_budget) narrow the window until the table fits.  Unless a window was set
 * explicitly, a key starts with w = 8 (13 MB, built in ~2 ms) and switches to the default after its first 4096
 * elements.  Results are identical. */
int pgpu_set_fixed_base_window(int w);
/* Table memory is bounded (round 3): per key and GPU by max_bytes_per_key (default 512 MiB, env
 * PGPU_FB_KEY_MAX_BYTES: the window narrows until the table fits), per GPU over ALL keys by max_bytes_per_device
 * (default 2 GiB, env PGPU_FB_MAX_BYTES: a new table first evicts the least recently used tables of other keys;
 * an evicted key rebuilds its table on its next encrypt).  0 leaves a limit unchanged.  Results never change. */
int pgpu_set_fixed_base_budget(size_t max_bytes_per_device, size_t max_bytes_per_key);
int pgpu_fixed_base_stats(int pool_index, size_t* live_bytes, uint64_t* evictions);
/* the table a key currently holds on a pool entry: window, bytes, build time in ms (0: none / still building) */
int pgpu_pubkey_fixed_base_info(const pgpu_pubkey* key, int pool_index, int* window, size_t* bytes, double* build_ms);

/* ---- Paillier private key: fused CRT decrypt ----
 * Replaces PrivateKey::decryptCRT + computeLfun + computeCRT (pri_key.cpp:114-157): per
 * ciphertext c (2*n_words words) two half-width exponentiations c^(p-1) mod p^2, c^(q-1) mod
 * q^2, the L function, *hp / *hq, and the CRT recombination; m has n_words words.
 * p and q have pq_words words each (either order: the smaller becomes p, pri_key.cpp:19-22). */
typedef struct pgpu_privkey pgpu_privkey;
int pgpu_privkey_create(const uint64_t* p, const uint64_t* q, int pq_words, pgpu_privkey** out);
void pgpu_privkey_destroy(pgpu_privkey* key);
int pgpu_paillier_decrypt_crt(const pgpu_privkey* key, const uint64_t* c, uint64_t* m,
                              size_t count);
int pgpu_paillier_decrypt_crt_dev(const pgpu_privkey* key, const uint64_t* d_c, uint64_t* d_m,
                                  size_t count, void* hip_stream);

/* ---- device buffers for callers that do not link the HIP runtime themselves ----
 * (the C++ ipcl:: layer keeps ciphertext batches resident in HBM between operations and feeds
 * them to the *_dev entry points on the default stream).  Copies are synchronous. */
int pgpu_dev_alloc(size_t bytes, void** out);
void pgpu_dev_free(void* d_ptr);
int pgpu_copy_h2d(void* d_dst, const void* h_src, size_t bytes);
int pgpu_copy_d2h(void* h_dst, const void* d_src, size_t bytes);

/* ---- pinned host memory ----
 * A caller buffer that lies inside a block from pgpu_host_alloc is the source / target of the DMA itself: every
 * host-pointer entry point, pgpu_batch_upload and pgpu_batch_download then skip their staging copies (a host thread moves
 * 8-10 GB/s between pageable and pinned memory, the link ~50 GB/s).  The reference's accelerator path does the same: HE-QAT
 * takes its operand buffers from the device driver's pinned allocator (module/heqat/heqat/bnops.c: qaeMemAllocNUMA).
 * pgpu_batch_upload from such a block only QUEUES the copy: the block must not be modified until pgpu_host_wait(ptr)
 * has returned (pgpu_host_free waits too; every other entry point is synchronous as before).  Results that land in a
 * block are complete on return.  Blocks are usable with every GPU of the pool and survive pgpu_shutdown. */
int pgpu_host_alloc(size_t bytes, void** out);
void pgpu_host_free(void* ptr);
int pgpu_host_wait(const void* ptr /* any address inside a block */);

/* ---- exponent schedules of private-key constants (see SIDE CHANNELS above) ---- */
typedef enum pgpu_exp_policy {
  PGPU_EXP_FIXED_WINDOW = 0, /* default: key-independent operation sequence                     */
  PGPU_EXP_SLIDING = 1       /* host-built sliding-window schedule of p-1 / q-1 (fewer products) */
} pgpu_exp_policy;
int pgpu_set_secret_exponent_policy(int policy);
int pgpu_get_secret_exponent_policy(void);
/* Window-table ACCESS of the split-form kernels (CRT decrypt, CT*PT and the key-less seam for 1024- to 3072-bit keys):
 * 0 (default) the entry is addressed by the exponent digit; 1 every entry of the table is read and the wanted one
 * selected, so that the address stream does not depend on the exponent -- what the reference's mbx_exp_mb8 does
 * (SURVEY Appendix B).  Costs 2^w x the table loads plus as many selects per multiplication (bench.py reports it).
 * DJN encrypt (round 4): with the policy on, hs^r runs as a fixed-base product over a SMALL-window table of its own
 * (w = 4, env PGPU_FB_MASKED_WINDOW 1..5: all 2^w entries of a window are read at every step and the wanted one is
 * selected) instead of the 2^12-entry windows addressed by the digits of r -- about 3x the indexed encrypt, 1/5 of a
 * masked square-and-multiply.  Both tables of a key may be live (2.4 MB + 203 MB for a 2048-bit key).  Not covered: the
 * full-width modexp_kernel (keys without a split form, PGPU_HENSEL=0).  Env PGPU_CT_GATHER=1. */
int pgpu_set_table_gather_policy(int masked);
int pgpu_get_table_gather_policy(void);

/* ---- sharded device-resident batches (SURVEY 8(f) N1 across the pool) ----
 * A pgpu_batch is [count][words] little-endian limbs living in GPU memory, cut into contiguous shards
 * over the pool (count == 1: one copy on every GPU, the reference's "vector (+) scalar" operand,
 * ciphertext.cpp:51-58).  Operations enqueue one launch per shard on the GPUs' batch streams and
 * return at once; pgpu_batch_download waits.  Batches are immutable once produced.
 * Ciphertext batches produced on the device stay in a device-side DOMAIN; the plain value only materialises in
 * pgpu_batch_download and callers never see the difference:
 *   - keys of 1024 / 2048 / 3072 bits (those with a split form): PAIR ROWS, c*R == a - (n*k)*b mod n^2 as 29-bit limbs
 *     (pgpu_batch_row_limbs) -- CT+CT is ONE pair product, CT+PT two half-width products, encrypt / CT*PT / CRT decrypt
 *     read and write the rows without conversion (ciphertext.cpp:135-141 does a multiply and a divide per CT+CT);
 *   - other keys, plaintext rows wider than n, PGPU_PAIR_ROWS=0: Montgomery-form words c*R mod n^2 -- CT+CT one
 *     full-width Montgomery product, encrypt emits the form for free, CRT decrypt absorbs it into its load constants.
 * Operations accept any mix (plain uploaded batches included) and convert on the way in.  An uploaded ciphertext batch
 * has 2 * n_words words and may hold values at and above n^2: the conversion on the way in runs over all 2 * n_words words,
 * whatever the value's size, so an operation reads such a row as its value modulo n^2 (held for CT+CT, CT*PT, negate, the
 * signed matvec / matmul and CRT decrypt at 2048 and 2051 bits; results are canonical, below n^2), and n^2
 * itself is the non-ciphertext 0 -- pgpu_batch_ct_negate and the signed calls refuse it as PGPU_ERR_NOT_INVERTIBLE. */
typedef struct pgpu_batch pgpu_batch;
int pgpu_batch_create(size_t count, int words, pgpu_batch** out);            /* uninitialised */
int pgpu_batch_upload(const uint64_t* host, size_t count, int words, size_t stride, pgpu_batch** out);
int pgpu_batch_download(const pgpu_batch* b, uint64_t* host /* [count][words] */);
/* Download that does not hold the caller (round 4): returns at once with a ticket; a worker of the pool runs the conversion
 * (if the batch is in a device-side domain) and queues the copy once the batch's kernels have finished -- never earlier, so
 * that it cannot block the copy engine for other lanes.  pgpu_ticket_wait blocks until the data has arrived, returns the
 * status of the download and frees the ticket.  `b` and `host` must stay alive until then.  With buffers from
 * pgpu_host_alloc this is what lets ONE thread pipeline whole host-to-host steps over two lanes (bench.py:
 * end_to_end_pipelined). */
/* Download with the rows `host_stride` words apart (the words between rows are overwritten with ZEROS -- write per-row
 * headers after the call): lets a host layer lay results out with room for its own per-row headers and use them in place
 * (the ipcl:: layer's BigNumbers point into the pinned block).  Pinned targets, one-GPU pools, plain or pair-row batches;
 * otherwise PGPU_ERR_UNSUPPORTED. */
int pgpu_batch_download_strided(const pgpu_batch* b, uint64_t* host, size_t host_stride_words);
/* 1: the batch belongs to the device pool that is up now; 0: its pool has been shut down (pgpu_shutdown, also followed by
 * a new pgpu_init*): every operation refuses it, only pgpu_batch_destroy takes it.  Lets a host layer that caches device
 * copies of caller data (the ipcl:: layer: injected randomness, texts uploaded at construction) fall back to its host
 * copy instead of failing. */
int pgpu_batch_is_current(const pgpu_batch* b);
typedef struct pgpu_ticket pgpu_ticket;
int pgpu_batch_download_async(const pgpu_batch* b, uint64_t* host /* [count][words] */, pgpu_ticket** out);
int pgpu_ticket_wait(pgpu_ticket* t);
void pgpu_batch_destroy(pgpu_batch* b);
size_t pgpu_batch_count(const pgpu_batch* b);
int pgpu_batch_words(const pgpu_batch* b);
int pgpu_batch_is_montgomery(const pgpu_batch* b);   /* 1: a device-side domain (Montgomery words or pair rows), 0: plain */
/* limbs per row when the batch is stored as PAIR ROWS (round 3; csrc/kargs.hpp), else 0.  Ciphertext batches produced
 * on the device for keys of 1024 / 2048 / 3072 bits are pairs (a, b) of 29-bit limbs with c*R == a - (n*k)*b mod n^2 --
 * the register image of the split-form kernels: CT+CT is ONE pair product, CT+PT two half-width products, encrypt /
 * CT*PT / CRT decrypt read and write the rows without any conversion.  PGPU_PAIR_ROWS=0 keeps Montgomery words. */
int pgpu_batch_row_limbs(const pgpu_batch* b);
/* Batch lanes: every GPU of the pool has pgpu_batch_lanes() (4) batch streams, so that many independent chains of
 * resident batches can be in flight at once (their kernels share the chip: a wavefront that is alone on a SIMD issues
 * ~8 % slower than two, and the sequential-halves kernels -- 11-17 % fewer instructions -- need 16384 ciphertexts in
 * flight to reach every SIMD).  Uploads and pgpu_batch_create take the calling thread's lane (the first thread of the
 * process that uploads gets lane 0, further threads the next lanes round-robin; pgpu_set_batch_lane overrides); every result
 * inherits the lane of the operation's first operand; operands of another lane are ordered in by events.
 * A thread that CHOOSES its lanes (pgpu_set_batch_lane) is taken to pipeline -- to keep several lanes fed without waiting in
 * between: what its launches look like depends on whether the neighbour lanes are busy when they are queued (the adaptive
 * policy, pgpu_decrypt_kernel_form_ex: part-chip launches side by side).  Threads on the round-robin lanes are synchronous
 * API callers (upload, operation, download): their lanes idle during the host part of every call, so their launches keep
 * the lone caller's full-chip forms and simply overlap one thread's copies and host work with another's kernels. */
int pgpu_set_batch_lane(int lane /* 0 .. pgpu_batch_lanes() - 1 */);
int pgpu_batch_lane(const pgpu_batch* b);
int pgpu_batch_lanes(void);
/* c = Enc(m; r): m, r batches of `count` elements (PublicKey::encrypt, pub_key.cpp:112-129) */
int pgpu_batch_encrypt(const pgpu_pubkey* key, const pgpu_batch* m, const pgpu_batch* r, int r_bits,
                       pgpu_batch** c);
/* m = Dec(c) (PrivateKey::decrypt CRT path, pri_key.cpp:65-90,114-157) */
int pgpu_batch_decrypt_crt(const pgpu_privkey* key, const pgpu_batch* c, pgpu_batch** m);
/* out = a*b mod n^2 under `key` (CipherText + CipherText, ciphertext.cpp:35-72); b may hold one element */
int pgpu_batch_ct_add(const pgpu_pubkey* key, const pgpu_batch* a, const pgpu_batch* b, pgpu_batch** out);
/* out = a * (1 + n*m) mod n^2 (CipherText + PlainText, ciphertext.cpp:75-80: g^m without obfuscator, then the
 * product -- here fused in one launch, no host loop); m may hold one element */
int pgpu_batch_ct_add_plain(const pgpu_pubkey* key, const pgpu_batch* a, const pgpu_batch* m, pgpu_batch** out);
/* out = a^e mod n^2 (CipherText * PlainText, ciphertext.cpp:83-106); e may hold one element */
int pgpu_batch_ct_mul(const pgpu_pubkey* key, const pgpu_batch* a, const pgpu_batch* e, int e_bits,
                      pgpu_batch** out);
/* Encrypted matrix-vector product (an encrypted linear layer, a weighted aggregate, a dot product): x a resident
 * ciphertext batch of cols = pgpu_batch_count(x) elements (pair rows, or uploaded plain ciphertext words: converted on
 * the way in), w a plain uploaded batch of rows*cols exponents, row-major, each < 2^e_bits (bits at and above e_bits are
 * ignored):
 *     out[i] = prod_j x[j]^w[i*cols + j] mod n^2           i.e. Dec(out[i]) = sum_j w[i][j] * Dec(x[j]) mod n
 * One simultaneous fixed-window multi-exponentiation instead of rows*cols pgpu_batch_ct_mul terms and a tree of
 * pgpu_batch_ct_add: the window tables of the x[j] are built once and shared by all rows, the e_bits squarings are done
 * once per output ("Encrypted matrix-vector product").  The result is an ordinary resident ciphertext batch of
 * `rows` elements on the lane of x.
 * PGPU_ERR_INVALID_PARAM: null / stale handles, rows == 0, count(w) != rows*cols, e_bits < 1 or wider than the rows of w.
 * PGPU_ERR_UNSUPPORTED: keys without pair rows (beyond 3072 bits; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0), pools of more than one
 * GPU, and -- SIDE CHANNELS -- the masked table-gather policy: the tables are indexed by digits of the PLAINTEXT matrix w
 * (never by key material or by anything encrypted), which is the indexed access of the default policy; with
 * pgpu_set_table_gather_policy(1) the call is refused rather than run with an access pattern the policy excludes. */
int pgpu_batch_ct_matvec(const pgpu_pubkey* key, const pgpu_batch* x, const pgpu_batch* w, size_t rows, int e_bits,
                         pgpu_batch** out);
/* What a call of this shape would run (host-side query, needs no device): the window width (1..6), the number of column
 * slices (1..cols; each slice of a row is one group of lanes and runs its own squarings, the partial products are folded
 * afterwards) and the bytes of the shared window table (cols * 2^window pair rows).  The rule is policy.hpp: matvec_*;
 * PGPU_MATVEC_WINDOW / PGPU_MATVEC_SLICES force the two values.  PGPU_ERR_UNSUPPORTED: no pair rows for keys of key_bits. */
int pgpu_ct_matvec_plan(int key_bits, size_t rows, size_t cols, int e_bits, int* window, int* slices, size_t* table_bytes);
/* Encrypted segmented sum (a histogram, a per-key aggregate, a pooling step): x a resident ciphertext batch of
 * cols = pgpu_batch_count(x) elements (pair rows, or uploaded plain ciphertext words: converted on the way in), ids a HOST
 * array of groups*cols segment numbers, row-major:
 *     out[g*n_segments + s] = prod_{ j : ids[g*cols + j] == s } x[j] mod n^2     i.e. Dec(out[g][s]) = sum of those Dec(x[j]) mod n
 * groups > 1: the same x under several groupings (one histogram per feature over the same samples).  An id equal to
 * PGPU_SEGMENT_NONE leaves the element out of that group; an empty segment yields the ciphertext 1, as an all-zero matrix
 * row does in pgpu_batch_ct_matvec.  The host sorts the element numbers by segment, cuts every segment into chunks (one
 * product chain each) and folds the partial products of long segments level by level with the same kernel (DESIGN.md:
 * "Encrypted segmented sum").  The result is an ordinary resident ciphertext batch of groups*n_segments elements on the
 * lane of x; ids may be reused as soon as the call returns.
 * PGPU_ERR_INVALID_PARAM: null / stale handles, groups == 0, n_segments == 0, ciphertext width mismatch, a batch of another
 * key, an id >= n_segments other than PGPU_SEGMENT_NONE, groups*cols or groups*n_segments beyond what the call addresses.
 * PGPU_ERR_UNSUPPORTED: keys without pair rows (beyond 3072 bits; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0), pools of more than one
 * GPU, and -- SIDE CHANNELS -- the masked table-gather policy: the rows of x are addressed by the caller's PLAINTEXT ids
 * (never by key material or by anything encrypted), which is the indexed access of the default policy; with
 * pgpu_set_table_gather_policy(1) the call is refused rather than run with an access pattern the policy excludes.
 * All refusals are decided on the host before any launch and leave *out untouched. */
#define PGPU_SEGMENT_NONE 0xFFFFFFFFu
int pgpu_batch_ct_segment_sum(const pgpu_pubkey* key, const pgpu_batch* x, const uint32_t* ids, size_t groups,
                              size_t n_segments, pgpu_batch** out);
/* What a call of this shape would run (host-side query, needs no device): elements = the ids that are not
 * PGPU_SEGMENT_NONE, segments = groups * n_segments, longest_segment = the elements of the fullest segment.  chunk: the
 * entries one product chain multiplies; levels: the launches, ceil(log_chunk(longest_segment)), at least 1.  The rule is
 * policy.hpp: segsum_*; PGPU_SEGSUM_CHUNK=c (c >= 2) forces the chunk.
 * PGPU_ERR_UNSUPPORTED: no pair rows for keys of key_bits. */
int pgpu_ct_segment_sum_plan(int key_bits, size_t elements, size_t segments, size_t longest_segment, int* chunk, int* levels);
/* Encrypted segmented prefix sum (the cumulative sum over the bins of every histogram, a running total, a CDF over
 * encrypted values): x a resident ciphertext batch of count = rows * seg_len elements (pair rows, or uploaded plain
 * ciphertext words: converted on the way in), read as [rows][seg_len]; the scan is inclusive:
 *     out[r][t] = prod_{ u <= t } x[r][u] mod n^2     i.e. Dec(out[r][t]) = sum_{u <= t} Dec(x[r][u]) mod n
 * and with PGPU_SCAN_REVERSE in flags the product runs over u >= t (suffix sums: the right-hand side of every split).
 * The result is an ordinary resident ciphertext batch of count elements in pair rows on the lane of x -- the layout
 * [groups][n_segments] of a pgpu_batch_ct_segment_sum result is scanned with seg_len = n_segments.  A row of at most
 * `chunk` entries is one product chain (seg_len - 1 products, one launch); a longer row is cut into chunks: the chunk
 * totals are multiplied up, scanned by the same procedure, and every chunk is walked again from the scanned total before
 * it ("Encrypted segmented prefix sum"), about 2 * count products.
 * PGPU_ERR_INVALID_PARAM: null / stale handles, seg_len == 0, count(x) % seg_len != 0, a flag bit other than
 * PGPU_SCAN_REVERSE, ciphertext width mismatch, a batch of another key, more chunks than a 32-bit carry index addresses.
 * PGPU_ERR_UNSUPPORTED: keys without pair rows (beyond 3072 bits; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0), pools of more than one
 * GPU, and the masked table-gather policy.  SIDE CHANNELS: the address stream of this call depends only on rows, seg_len
 * and the plan -- no index list, nothing derived from a value; the refusal under pgpu_set_table_gather_policy(1) is kept
 * for symmetry with pgpu_batch_ct_matvec and pgpu_batch_ct_segment_sum, so that one rule covers the aggregation calls.
 * All refusals are decided on the host before any launch and leave *out untouched. */
#define PGPU_SCAN_REVERSE 1u
int pgpu_batch_ct_segment_scan(const pgpu_pubkey* key, const pgpu_batch* x, size_t seg_len, unsigned flags, pgpu_batch** out);
/* What a call of this shape would run (host-side query, needs no device).  chunk: the entries one product chain walks
 * (seg_len itself when one chain per row is the plan); levels: the depth of the hierarchy, 1 when seg_len <= chunk -- a
 * call runs 2 * levels - 1 launches; products: the pair products of all launches, padding excluded.  The rule is
 * policy.hpp: segscan_*; PGPU_SEGSCAN_CHUNK=c (c >= 2) forces the chunk, read at every call.
 * PGPU_ERR_UNSUPPORTED: no pair rows for keys of key_bits.  PGPU_ERR_INVALID_PARAM: rows == 0, seg_len == 0, more chunks
 * than a 32-bit carry index addresses. */
int pgpu_ct_segment_scan_plan(int key_bits, size_t rows, size_t seg_len, int* chunk, int* levels, size_t* products);
/* Encrypted slot packing ("cipher compressing": pack before decrypt): x a resident ciphertext batch of count = rows *
 * seg_len elements (pair rows, or uploaded plain ciphertext words: converted on the way in), read as [rows][seg_len]:
 *     out[r] = prod_t x[r][t]^(2^(slot_bits * t)) mod n^2     i.e. Dec(out[r]) = sum_t Dec(x[r][t]) * 2^(slot_bits * t) mod n
 * -- one ciphertext whose plaintext carries seg_len slots of slot_bits bits, slot 0 the least significant: the key holder
 * decrypts rows ciphertexts where it decrypted count, and 1 / seg_len of the bytes travel.  The result is an ordinary
 * resident ciphertext batch of rows elements in pair rows on the lane of x, usable by every other operation; x is left
 * unchanged.  One launch, one Horner chain per row: (seg_len - 1) * (slot_bits + 1) pair products ("Encrypted
 * slot packing"); seg_len == 1 is a copy (it converts, but runs no product).
 * SLOTS: nothing here looks at the values.  A slot value of 2^slot_bits or more carries into its neighbour, exactly as in
 * an integer sum; headroom for sums taken AFTER packing (pgpu_batch_ct_add of packed rows adds slot-wise) is the caller's
 * choice of slot_bits: k packed rows added need slot_bits >= bits of a value + ceil(log2 k).
 * PGPU_ERR_INVALID_PARAM: null / stale handles, seg_len == 0, count(x) % seg_len != 0, slot_bits < 1, seg_len * slot_bits
 * > bitlen(n) - 1 (a pack that wraps modulo n is never meant), ciphertext width mismatch, a batch of another key.
 * PGPU_ERR_UNSUPPORTED: keys without pair rows (beyond 3072 bits; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0), pools of more than one
 * GPU, and the masked table-gather policy.  SIDE CHANNELS: the address stream of this call depends only on rows and
 * seg_len; the refusal under pgpu_set_table_gather_policy(1) is kept so that one rule covers the aggregation calls.
 * All refusals are decided on the host before any launch and leave *out untouched. */
int pgpu_batch_ct_pack(const pgpu_pubkey* key, const pgpu_batch* x, size_t seg_len, int slot_bits, pgpu_batch** out);
/* What a call of this shape would run (host-side query, needs no device).  lanes, limbs: the (G, K) form of the launch;
 * products = rows * (seg_len - 1) * (slot_bits + 1).  The capacity bound is taken as key_bits - 1.
 * PGPU_ERR_INVALID_PARAM: key_bits < 1, rows == 0, seg_len == 0, slot_bits < 1, seg_len * slot_bits > key_bits - 1, a product
 * count beyond size_t.  PGPU_ERR_UNSUPPORTED: no pair rows for keys of key_bits. */
int pgpu_ct_pack_plan(int key_bits, size_t rows, size_t seg_len, int slot_bits, int* lanes, int* limbs, size_t* products);
/* Encrypted sparse matrix-vector product (a neighbourhood aggregation over a graph, a sparse or pruned linear layer, a
 * convolution as a banded matrix -- pgpu_batch_ct_conv2d below does that without the index list --, SUM(v*x) GROUP BY id): x a resident ciphertext batch of cols = pgpu_batch_count(x)
 * elements (pair rows, or uploaded plain ciphertext words: converted on the way in), the plaintext matrix A in CSR form:
 * row_ptr[rows + 1] and col_idx[nnz] HOST arrays, w a plain uploaded batch of nnz = row_ptr[rows] exponents in CSR order,
 * each < 2^e_bits (bits at and above e_bits are ignored):
 *     out[i] = prod_{ row_ptr[i] <= t < row_ptr[i+1] } x[col_idx[t]]^w[t] mod n^2
 *     i.e. Dec(out[i]) = sum_t w[t] * Dec(x[col_idx[t]]) mod n
 * The entries of a row need not be sorted by column; a column named twice in a row contributes twice; a zero weight
 * contributes 1; an empty row yields the ciphertext 1, as an empty segment and an all-zero matvec row do.  Negative
 * weights have no encoding: pass w mod n.  The window tables of the x[j] are built once and shared by all rows; every row
 * is cut into chains of at most `chunk` entries, each one multi-exponentiation with its own e_bits squarings, and the
 * partial products of the rows of several chains are folded level by level ("Encrypted sparse matrix-vector
 * product").  The result is an ordinary resident ciphertext batch of `rows` elements in pair rows on the lane of x; x is
 * left unchanged; row_ptr and col_idx may be reused as soon as the call returns.
 * PGPU_ERR_INVALID_PARAM: null / stale handles, rows == 0, row_ptr[0] != 0, row_ptr not non-decreasing, nnz == 0,
 * count(w) != nnz, w not a plain uploaded batch, a col_idx[t] >= cols, e_bits < 1 or wider than the rows of w, ciphertext
 * width mismatch, a batch of another key, rows, nnz or the number of chains beyond what 32-bit descriptors address (2^31).
 * PGPU_ERR_UNSUPPORTED: keys without pair rows (beyond 3072 bits; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0), pools of more than one
 * GPU, and -- SIDE CHANNELS -- the masked table-gather policy: the tables are indexed by the caller's PLAINTEXT column
 * numbers and by digits of the PLAINTEXT weights w (never by key material or by anything encrypted), which is the indexed
 * access of the default policy; with pgpu_set_table_gather_policy(1) the call is refused rather than run with an access
 * pattern the policy excludes.
 * All refusals are decided on the host before any launch and leave *out untouched. */
int pgpu_batch_ct_spmv(const pgpu_pubkey* key, const pgpu_batch* x, const uint64_t* row_ptr, const uint32_t* col_idx,
                       const pgpu_batch* w, size_t rows, int e_bits, pgpu_batch** out);
/* What a call of this shape would run (host-side query, needs no device).  window: the window width (1..6); chunk: the
 * entries one chain multiplies in per window; levels: 1 (the multi-exponentiation) plus the fold launches that the longest
 * row needs (the table build is one launch more); table_bytes: cols * 2^window pair rows -- the table covers EVERY column
 * of x; products: the pair products of the call, table included, counting the longest row cut by the chunk and the
 * other rows as equally long (exact while longest_row <= chunk and for rows of one length, an estimate otherwise).  The rule is policy.hpp: spmv_*;
 * PGPU_SPMV_WINDOW / PGPU_SPMV_CHUNK (c >= 1) force the two values, read at every call.
 * PGPU_ERR_INVALID_PARAM: key_bits < 1, rows == 0, cols == 0, nnz == 0, longest_row == 0 or > nnz, nnz > rows * longest_row,
 * e_bits < 1, rows or nnz of 2^31 or more.  PGPU_ERR_UNSUPPORTED: no pair rows for keys of key_bits. */
int pgpu_ct_spmv_plan(int key_bits, size_t rows, size_t cols, size_t nnz, size_t longest_row, int e_bits,
                      int* window, int* chunk, int* levels, size_t* table_bytes, size_t* products);
/* Encrypted weighted sum of K resident batches (a federated average: K clients send one encrypted vector each, the server
 * aggregates ACROSS them): xs[k] resident ciphertext batches of one common count under `key` (pair rows, or uploaded plain
 * ciphertext words: converted on the way in; any mix within one call), one plaintext weight per BATCH:
 *     out[i] = prod_k xs[k][i]^(a_k) mod n^2
 *     i.e. Dec(out[i]) = sum_k a_k * Dec(xs[k][i]) mod n
 * weights: HOST words, [n_terms][w_words] little-endian, of any width up to w_words words (a mod n for a negative a is a
 * legal, full-width weight), consumed before the call returns; NULL: every weight is 1, the plain sum.  The device never
 * reads them: the host turns them into one bit-serial schedule that is the same for every element -- one squaring per bit
 * below the top one, one product per set bit, nothing for a zero bit, the squarings shared by all K terms -- and cuts the
 * terms into slices that run side by side where the elements alone leave the chip empty, folded by one more launch
 * ("Encrypted weighted sum of K resident batches").  The same handle may appear more than once and contributes
 * once per appearance; a zero weight contributes 1 and its batch is never read; if every weight is zero every row is the
 * ciphertext 1, as an empty segment and an empty spmv row are; n_terms == 1 with weight 1 is a copy.  The result is an
 * ordinary resident ciphertext batch of count elements in pair rows on the lane of xs[0] (operands of other lanes are
 * ordered in by events, as for pgpu_batch_ct_add); every xs[k] is left unchanged.
 * PGPU_ERR_INVALID_PARAM: null / stale handles, n_terms == 0 or above 65535, counts that differ, ciphertext width
 * mismatch, a batch of another key, w_words < 1 with non-null weights, a schedule of 2^31 steps or more.
 * PGPU_ERR_UNSUPPORTED: keys without pair rows (beyond 3072 bits; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0), pools of more than one
 * GPU, and -- SIDE CHANNELS -- the masked table-gather policy: the schedule and the row addresses depend on the caller's
 * PLAINTEXT weights only (never on key material or on anything encrypted); with pgpu_set_table_gather_policy(1) the call
 * is refused all the same, which keeps one rule for the aggregation calls.
 * All refusals are decided on the host before any launch and leave *out untouched; there is no element-wise fall-back. */
int pgpu_batch_ct_weighted_sum(const pgpu_pubkey* key, const pgpu_batch* const* xs, size_t n_terms,
                               const uint64_t* weights /* HOST, [n_terms][w_words] little-endian, or NULL: all ones */,
                               int w_words, pgpu_batch** out);
/* What a call of this shape would run (host-side query, needs no device).  lanes, limbs: the (G, K) form of the first
 * launch; slices: the non-empty slices of the terms (1: one launch; more: one launch over all slices plus one fold
 * launch); steps: the schedule length of the longest slice; products: the pair products of the call, count * ((bits - 1)
 * squarings + (set bits - 1) products per slice + (slices - 1) for the fold) -- exact, padding excluded.  The rule is
 * policy.hpp: wsum_*; PGPU_WSUM_SLICES=s / PGPU_WSUM_WIDE=0|1 force the slices and the form, read at every call.
 * PGPU_ERR_INVALID_PARAM: key_bits < 1, count == 0, n_terms == 0 or above 65535, w_words < 1 with non-null weights, a
 * schedule of 2^31 steps or more, a product count beyond size_t.  PGPU_ERR_UNSUPPORTED: no pair rows for keys of key_bits. */
int pgpu_ct_weighted_sum_plan(int key_bits, size_t count, size_t n_terms, const uint64_t* weights_or_null, int w_words,
                              int* lanes, int* limbs, int* slices, size_t* steps, size_t* products);
/* Encrypted matrix product (an encrypted linear layer applied to a minibatch, a per-class gradient): x a resident
 * ciphertext batch of n_vec*cols elements (pair rows, or uploaded plain ciphertext words: converted on the way in), read as
 * n_vec vectors of cols = pgpu_batch_count(x) / n_vec elements; w a plain uploaded batch of rows*cols exponents, row-major
 * as in pgpu_batch_ct_matvec, each < 2^e_bits (bits at and above e_bits are ignored):
 *     flags == 0:               x read as [n_vec][cols], out as [n_vec][rows]
 *         out[v*rows + i] = prod_j x[v*cols + j]^w[i*cols + j] mod n^2          (Y = X * W^T, the nn.Linear convention)
 *     PGPU_MATMUL_TRANSPOSED:   x read as [cols][n_vec], out as [rows][n_vec]
 *         out[i*n_vec + v] = prod_j x[j*n_vec + v]^w[i*cols + j] mod n^2        (Y = W * X)
 * i.e. Dec(out) = W * Dec(x) mod n for every vector.  With n_vec == 1 both layouts are pgpu_batch_ct_matvec; an all-zero
 * row of w yields the ciphertext 1; negative weights have no encoding (pass w mod n).  The schedule of an output is the
 * matvec's; the vectors are walked in tiles -- one tile's window tables are built, used by all rows, and the table block is
 * reused by the next tile -- so that the tables stay under the cap of the matvec at the window the product count wants,
 * however many vectors there are ("Encrypted matrix product"; what pgpu_batch_ct_spmv needs n_vec*rows*cols
 * column numbers and as many weights for, and one table over all of x).  The result is an ordinary resident ciphertext
 * batch of n_vec*rows elements in pair rows on the lane of x; x is left unchanged.
 * PGPU_ERR_INVALID_PARAM: null / stale handles, n_vec == 0, rows == 0, count(x) % n_vec != 0, count(w) != rows*cols, w not a
 * plain uploaded batch, e_bits < 1 or wider than the rows of w, a flag bit other than PGPU_MATMUL_TRANSPOSED, ciphertext
 * width mismatch, a batch of another key, n_vec*rows beyond size_t.
 * PGPU_ERR_UNSUPPORTED: keys without pair rows (beyond 3072 bits; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0), pools of more than one
 * GPU, and -- SIDE CHANNELS -- the masked table-gather policy: the tables are indexed by digits of the PLAINTEXT matrix w
 * (never by key material or by anything encrypted), as in pgpu_batch_ct_matvec.
 * All refusals are decided on the host before any launch and leave *out untouched. */
#define PGPU_MATMUL_TRANSPOSED 1u
int pgpu_batch_ct_matmul(const pgpu_pubkey* key, const pgpu_batch* x, const pgpu_batch* w, size_t n_vec, size_t rows,
                         int e_bits, unsigned flags, pgpu_batch** out);
/* What a call of this shape would run (host-side query, needs no device): the window width (1..6), the vectors of a tile
 * (1..n_vec; the call makes ceil(n_vec / tile) passes, the last one over the vectors that remain), the column slices of a
 * full pass (1..cols; a short last pass has the slices of its own size), the bytes of the table block (tile * cols *
 * 2^window pair rows) and the pair products of the whole call: per pass over t vectors t*cols*(2^w - 2) for the tables,
 * t*rows*S*e_bits squarings, t*rows*cols*ceil(e_bits / w) products by table entries, t*rows*(S - 1) for the fold.  Every
 * pass is a table launch, a multiply launch and ceil(log2 S) fold launches.  The rule is policy.hpp: matmul_plan;
 * PGPU_MATMUL_WINDOW / PGPU_MATMUL_TILE / PGPU_MATMUL_SLICES force the three values, read at every call.
 * PGPU_ERR_INVALID_PARAM: a size or e_bits that is not positive, a product count beyond size_t.  PGPU_ERR_UNSUPPORTED: no
 * pair rows for keys of key_bits. */
int pgpu_ct_matmul_plan(int key_bits, size_t n_vec, size_t rows, size_t cols, int e_bits,
                        int* window, int* slices, size_t* tile, size_t* table_bytes, size_t* products);
/* Bucket-method encrypted matrix-vector product: few rows over very many columns, or weights of any width (a signed
 * weight sent as w mod n is full width).  x a resident ciphertext batch of cols elements (pair rows, or uploaded plain
 * ciphertext words: converted on the way in); w HOST memory, rows*cols weights of w_words little-endian 64-bit words each,
 * row-major, consumed before the call returns (the host cuts the digits, as pgpu_batch_ct_weighted_sum does):
 *     out[i] = prod_j x[j]^(w[i*cols + j] mod 2^e_bits) mod n^2,      1 <= e_bits <= 64 * w_words,
 * i.e. Dec(out) = W * Dec(x) mod n, bit for bit what pgpu_batch_ct_matvec returns.  A zero weight contributes 1 and an
 * all-zero row yields the ciphertext 1.  There are no window tables: every weight is cut into ceil(e_bits / c) digits of
 * c bits, the columns that share digit d of a (row, window) are multiplied into bucket d (a segmented sum: one product
 * per column and window whatever c is), the buckets are reduced to prod_d B_d^d by running products in two levels, and
 * the windows are combined by Horner ("Bucket-method matvec").  About rows * W * (cols + 2 * 2^c) products
 * instead of rows * cols * e_bits.  The result is an ordinary resident ciphertext batch of `rows` elements in pair rows
 * on the lane of x; x is left unchanged.  There is no fall-back to pgpu_batch_ct_matvec or to the element-wise route.
 * PGPU_ERR_INVALID_PARAM: null / stale handles, rows == 0, w_words < 1, e_bits outside 1 .. 64 * w_words, ciphertext width
 * mismatch, a batch of another key, rows * W * cols or rows * W * 2^c at or beyond 2^31 (what the descriptors address), a
 * bucket block of more than 4 GiB (a forced window, or c = 1 where no window fits the plan's 256 MiB cap), a plan beyond host memory.
 * PGPU_ERR_UNSUPPORTED: keys without pair rows (beyond 3072 bits; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0), pools of more than one
 * GPU, and -- SIDE CHANNELS -- the masked table-gather policy: the ciphertext rows are addressed by digits of the PLAINTEXT
 * weights (never by key material or by anything encrypted).
 * All refusals are decided on the host before any launch and leave *out untouched. */
int pgpu_batch_ct_matvec_bucket(const pgpu_pubkey* key, const pgpu_batch* x, const uint64_t* w, int w_words, size_t rows,
                                int e_bits, pgpu_batch** out);
/* What a call of this shape would run (host-side query, needs no device): the window c (1..10), the block b of the
 * first reduction level (a power of two, 1..2^c), the bytes of the bucket block (rows * W * 2^c pair rows, W =
 * ceil(e_bits / c)), and data-independent upper bounds of the pair products of the whole call -- rows*W*cols for the
 * buckets, rows*W*nb*2(b-1) and rows*W*(2(nb-1) + log2 b + nb) for the two reduction levels (nb = 2^c / b),
 * rows*(W-1)*(c+1) for Horner -- and of its depth, the products one after the other: the longest chain of every
 * accumulation level, the two reduction chains, the Horner chain.  The rule is policy.hpp: bucket_plan;
 * PGPU_BUCKET_WINDOW / PGPU_BUCKET_BLOCK force the two values, read at every call.
 * PGPU_ERR_INVALID_PARAM: a size or e_bits that is not positive, a product count beyond size_t.  PGPU_ERR_UNSUPPORTED: no
 * pair rows for keys of key_bits. */
int pgpu_ct_matvec_bucket_plan(int key_bits, size_t rows, size_t cols, int e_bits, int* window, int* block,
                               size_t* bucket_bytes, size_t* products, size_t* depth);
/* Encrypted 2-D convolution (a convolutional layer on encrypted images, a sliding-window or moving sum, sum pooling): x a
 * resident ciphertext batch of n_img*c_in*h*w elements (pair rows, or uploaded plain ciphertext words: converted on the way
 * in) read as [n_img][c_in][h][w]; w a plain uploaded batch of c_out*c_in*kh*kw exponents read as [c_out][c_in][kh][kw],
 * each < 2^e_bits (bits at and above e_bits are ignored).  With
 *     oh = (h + 2*pad_h - kh) / stride_h + 1 (floor),   ow likewise,
 *     out[n][co][oy][ox] = prod_{ci,ky,kx} x[n][ci][oy*stride_h + ky - pad_h][ox*stride_w + kx - pad_w]^w[co][ci][ky][kx] mod n^2,
 * a tap outside the image contributing 1 (zero padding): Dec(out) is the cross-correlation that
 * torch.nn.functional.conv2d computes, taken mod n.  h == kh == 1 is a 1-D convolution; sum pooling is the caller's reshape
 * (n_img' = n_img*c, c_in = c_out = 1, all-ones taps, e_bits = 1, stride equal to the kernel).  An all-zero filter yields the
 * ciphertext 1; negative weights have no encoding (pass w mod n).  Not offered: dilation, groups, a bias (that is
 * pgpu_batch_ct_add_plain on the result), and tiling inside one image.
 * The schedule of an output is the matmul's; the images are walked in tiles of whole images -- one tile's window tables are
 * built once, every tap of every output that reads a pixel addresses its table by arithmetic on the output position, and
 * the table block is reused by the next tile ("Encrypted 2-D convolution"; what pgpu_batch_ct_spmv needs
 * n_img*c_out*oh*ow*c_in*kh*kw column numbers and as many replicated weights for, and one table over all of x).  The
 * result is an ordinary resident ciphertext batch of n_img*c_out*oh*ow elements in pair rows on the lane of x, laid out
 * [n_img][c_out][oh][ow]: a second layer takes it as it is.  x is left unchanged.
 * PGPU_ERR_INVALID_PARAM: null / stale handles, a dimension or stride equal to 0, pad_h >= kh or pad_w >= kw (a window that
 * holds no element), kh > h + 2*pad_h or kw > w + 2*pad_w (no output), count(x) != n_img*c_in*h*w, count(w) !=
 * c_out*c_in*kh*kw, w not a plain uploaded batch, e_bits < 1 or wider than the rows of w, ciphertext width mismatch, a batch
 * of another key, a size product beyond size_t (an image or kernel side of 2^30 or more counts as one).
 * PGPU_ERR_UNSUPPORTED: keys without pair rows (beyond 3072 bits; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0), pools of more than one
 * GPU, and -- SIDE CHANNELS -- the masked table-gather policy: the tables are indexed by digits of the PLAINTEXT filters and
 * by positions derived from the shape (never by key material or by anything encrypted).
 * All refusals are decided on the host before any launch and leave *out untouched. */
typedef struct pgpu_conv2d_shape {
  size_t n_img, c_in, h, w, c_out, kh, kw, stride_h, stride_w, pad_h, pad_w;
} pgpu_conv2d_shape;
int pgpu_batch_ct_conv2d(const pgpu_pubkey* key, const pgpu_batch* x, const pgpu_batch* w, const pgpu_conv2d_shape* shape,
                         int e_bits, pgpu_batch** out);
/* What a call of this shape would run (host-side query, needs no device): the window width (1..6), the images of a tile
 * (1..n_img; the call makes ceil(n_img / tile) passes, the last one over the images that remain), the tap slices of a full
 * pass (1..c_in*kh*kw; a short last pass has the slices of its own size), the bytes of the table block (tile * c_in*h*w *
 * 2^window pair rows) and the pair products of the whole call: per pass over t images, with n_o = c_out*oh*ow and taps =
 * c_in*kh*kw, t*c_in*h*w*(2^w - 2) for the tables, t*n_o*S*e_bits squarings, t*n_o*taps*ceil(e_bits / w) products by table
 * entries (padded taps counted: they are multiplied by one), t*n_o*(S - 1) for the fold.  Every pass is a table launch, a
 * multiply launch and ceil(log2 S) fold launches.  The rule is policy.hpp: conv_plan; PGPU_CONV_WINDOW / PGPU_CONV_TILE /
 * PGPU_CONV_SLICES force the three values, read at every call.
 * PGPU_ERR_INVALID_PARAM: key_bits or e_bits < 1, a null shape, and what the call refuses of a shape alone: a dimension or
 * stride equal to 0, pad >= kernel, kernel > padded image, a size product or a product count beyond size_t.
 * PGPU_ERR_UNSUPPORTED: no pair rows for keys of key_bits. */
int pgpu_ct_conv2d_plan(int key_bits, const pgpu_conv2d_shape* shape, int e_bits, int* window, int* slices, size_t* tile,
                        size_t* table_bytes, size_t* products);

/* Ciphertext negation and subtraction: x (a, b) resident ciphertext batches of count elements under key (pair rows, or
 * uploaded plain ciphertext words: converted on the way in):
 *     negate   out[i] = x[i]^-1 mod n^2              i.e. Dec(out[i]) = -Dec(x[i]) mod n
 *     sub      out[i] = a[i] * b[i]^-1 mod n^2       i.e. Dec(out[i]) = Dec(a[i]) - Dec(b[i]) mod n
 * b has count(a) elements, or one (the broadcast pgpu_batch_ct_add allows: one inverse, multiplied into every a[i]).  The
 * result is an ordinary resident ciphertext batch of count elements in pair rows on the lane of the first operand
 * (operands of other lanes are ordered in by events, as for pgpu_batch_ct_add); the operands are left unchanged.  The
 * downloaded result is the canonical value: pow(c, -1, n^2), and a * pow(b, -1, n^2) mod n^2.
 * All inverses of a batch come from ONE modular inversion by simultaneous inversion ("Ciphertext negation and
 * subtraction"): a forward pass stores the running products of chains of `chunk` rows, the chain totals are inverted by the
 * same procedure, and every chain is walked back from the inverse of its total -- 3 * (count - 1) pair products for
 * negate, count more for sub (multiplied in by the last walk: no extra launch, no intermediate batch), where
 * pgpu_batch_ct_mul by n - 1 runs about 2400 per element of a 2048-bit key.  The one inversion is the HOST's: per call one
 * row travels down, the lane's stream is synchronised once, one row travels up.  That inversion is variable-time over a
 * product of ciphertexts, which is public data.
 * PGPU_ERR_INVALID_PARAM: null / stale handles, a null out, count(b) neither count(a) nor 1, ciphertext width mismatch, a
 * batch of another key, more chains than the descriptors address.
 * PGPU_ERR_UNSUPPORTED: keys without pair rows (beyond 3072 bits; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0), pools of more than one
 * GPU, and the masked table-gather policy.  SIDE CHANNELS: the address stream of these calls depends only on count and the
 * plan; the refusal under pgpu_set_table_gather_policy(1) is kept so that one rule covers the aggregation calls.
 * These refusals are decided on the host before any launch and leave *out untouched.
 * PGPU_ERR_NOT_INVERTIBLE: the product of the batch (for sub: of b) is not a unit modulo n -- an element is 0 or shares a
 * factor with n; neither is a ciphertext.  This ONE refusal FOLLOWS LAUNCHES: it is known when the host has the grand
 * total, after the forward passes.  It leaves *out untouched, frees what the call allocated, and the lane stays usable. */
int pgpu_batch_ct_negate(const pgpu_pubkey* key, const pgpu_batch* x, pgpu_batch** out);
int pgpu_batch_ct_sub(const pgpu_pubkey* key, const pgpu_batch* a, const pgpu_batch* b, pgpu_batch** out);
/* What a negate of this size would run (host-side query, needs no device; every output pointer may be NULL).  chunk: the
 * rows of one chain of the first level (the levels above it, which cannot fill the chip, are cut into pairs); levels: the
 * depth of the hierarchy, 1 when count <= chunk; launches: what the timing record shows as
 * PGPU_KERNEL_INVERT for pair-row input, a forward pass and a walk back per level -- count == 1 has nothing to multiply
 * forward and is one walk back; products: 3 * (count - 1), padding excluded.  The rule is policy.hpp: invert_*;
 * PGPU_INVERT_CHUNK=c (c >= 2) forces the chunk of every level, PGPU_INVERT_WIDE=0 / 1 its form, read at every call.
 * PGPU_ERR_UNSUPPORTED: no pair rows for keys of key_bits.  PGPU_ERR_INVALID_PARAM: key_bits < 1, count == 0, more chains
 * than the descriptors address. */
int pgpu_ct_negate_plan(int key_bits, size_t count, int* chunk, int* levels, int* launches, size_t* products);

/* Signed-weight encrypted matrix-vector and matrix products on resident ciphertexts: pgpu_batch_ct_matvec and
 * pgpu_batch_ct_matmul for weights that may be negative,
 *     out[i] = prod_j x[j]^W[i][j] mod n^2,      W[i][j] a SIGNED integer in two's complement in e_bits bits
 * (1 <= e_bits <= 64 * words(w)): bit e_bits - 1 of a stored weight is its sign, bits at and above e_bits are ignored.
 * `w` is a plain uploaded batch of rows * cols weights, row-major; an int64 array goes in as it is (words = 1, e_bits up
 * to 64), wider weights are multi-word two's complement.  The downloaded result is the canonical value, the product of
 * Python's pow(x[j], W[i][j], n * n), where a negative exponent goes through pow(x[j], -1, n * n); under decryption
 * Dec(out) = W * Dec(x) mod n.  The matmul takes n_vec vectors and the PGPU_MATMUL_TRANSPOSED flag in exactly the layouts
 * of pgpu_batch_ct_matmul.
 * Schedule ("Signed-weight matvec and matmul"): x^-1 by the batched inversion of pgpu_batch_ct_negate, once per
 * call over all elements (launches of kind PGPU_KERNEL_INVERT, one host round trip); a window table of 2^w + 1 rows per
 * element over [x ; x^-1] -- one, x^1 .. x^h, x^-1 .. x^-h, h = 2^(w-1) --, as many products to build as the unsigned
 * table; the multi-exponentiation of the unsigned call on the radix-2^w Booth digits of the weight, as many as it has
 * unsigned digits; the unchanged fold (kinds PGPU_KERNEL_MATVEC / PGPU_KERNEL_MATMUL).  A signed call so costs the
 * unsigned one plus 3 * (elements - 1) products, where sub(matvec(x, W+), matvec(x, W-)) runs two of them.
 * The refusals are those of the unsigned calls, decided on the host before any launch, *out untouched:
 * PGPU_ERR_INVALID_PARAM for null / stale handles, size and width mismatches, e_bits outside 1 .. 64 * words(w), a matrix
 * that is no plain uploaded batch, a batch of another key; PGPU_ERR_UNSUPPORTED for keys without pair rows, pools of more
 * than one GPU and the masked table-gather policy (the tables are indexed by digits of the plaintext matrix).
 * PGPU_ERR_NOT_INVERTIBLE: an element of x is no unit modulo n^2.  As for negate this ONE refusal FOLLOWS LAUNCHES (the
 * inversion's forward passes); nothing is handed out and the lane stays usable.  There is no fall-back to another route. */
int pgpu_batch_ct_matvec_signed(const pgpu_pubkey* key, const pgpu_batch* x, const pgpu_batch* w, size_t rows, int e_bits,
                                pgpu_batch** out);
int pgpu_batch_ct_matmul_signed(const pgpu_pubkey* key, const pgpu_batch* x, const pgpu_batch* w, size_t n_vec, size_t rows,
                                int e_bits, unsigned flags, pgpu_batch** out);
/* What the signed calls would run (host-side queries, need no device; every output pointer may be NULL): slices and tile
 * by the unsigned rules, the window that minimises the same product count among those whose table of 2^w + 1 rows per
 * element fits the unsigned calls' cap, table_bytes = elements of a pass * (2^w + 1) * row bytes, and products = the
 * unsigned count + 3 * (elements of the call - 1) for the inversion.  PGPU_MATVEC_WINDOW / _SLICES and PGPU_MATMUL_WINDOW /
 * _TILE / _SLICES force the signed calls too, read at every call.  Errors as pgpu_ct_matvec_plan / pgpu_ct_matmul_plan. */
int pgpu_ct_matvec_signed_plan(int key_bits, size_t rows, size_t cols, int e_bits, int* window, int* slices,
                               size_t* table_bytes, size_t* products);
int pgpu_ct_matmul_signed_plan(int key_bits, size_t n_vec, size_t rows, size_t cols, int e_bits,
                               int* window, int* slices, size_t* tile, size_t* table_bytes, size_t* products);

/* Signed-weight encrypted 2-D convolution and sparse matrix-vector product on resident ciphertexts: pgpu_batch_ct_conv2d
 * and pgpu_batch_ct_spmv for weights that may be negative (a CNN filter, a graph Laplacian),
 *     out[n][co][oy][ox] = prod_{ci,ky,kx} x[n][ci][oy*sh + ky - ph][ox*sw + kx - pw]^w[co][ci][ky][kx] mod n^2
 *     out[i] = prod_{ row_ptr[i] <= t < row_ptr[i+1] } x[col_idx[t]]^w[t] mod n^2,
 * every weight a SIGNED integer in two's complement in e_bits bits exactly as for pgpu_batch_ct_matvec_signed: bit
 * e_bits - 1 of a stored weight is its sign, bits at and above e_bits are ignored, 1 <= e_bits <= 64 * words(w), an int64
 * array goes in as it is.  Layouts, shape rules, zero padding (a tap outside the image contributes one, whatever its
 * weight's sign), strides, empty rows and "a column named twice contributes twice" (with weights a and -a: the ciphertext
 * 1) are those of the unsigned calls.  The downloaded result is the canonical value, the product of Python's
 * pow(x, w, n * n), where a negative exponent goes through pow(x, -1, n * n); it is an ordinary resident batch on the lane
 * of x, and x is left unchanged.
 * Schedule ("Signed-weight conv2d and spmv"): x^-1 by the batched inversion of pgpu_batch_ct_negate, ONCE per call
 * over ALL elements of x and before the first pass (launches of kind PGPU_KERNEL_INVERT, one host round trip); then the
 * unsigned call's launches on a window table of 2^w + 1 rows per element over [x ; x^-1] and on the radix-2^w Booth digits
 * of the weights -- per pass of whole images for the convolution, once over every column for the sparse product -- and the
 * unchanged folds (kinds PGPU_KERNEL_CONV / PGPU_KERNEL_SPMV).  A signed call so costs the unsigned one plus
 * 3 * (elements of x - 1) products, where sub(conv2d(x, W+), conv2d(x, W-)) runs two of them.
 * pgpu_batch_ct_spmv_signed inverts EVERY element of x, referenced by a column index or not: an element of x that is no
 * unit refuses the call also where no entry of the matrix names its column.
 * The refusals are those of the unsigned calls, decided on the host before any launch, *out untouched
 * (PGPU_ERR_INVALID_PARAM / PGPU_ERR_UNSUPPORTED as listed at pgpu_batch_ct_conv2d and pgpu_batch_ct_spmv; the masked
 * table-gather policy refuses both).  PGPU_ERR_NOT_INVERTIBLE: an element of x is no unit modulo n^2.  As for negate this
 * ONE refusal FOLLOWS LAUNCHES (the inversion's forward passes; none of kind CONV / SPMV); nothing is handed out and the
 * lane stays usable.  There is no fall-back to another route. */
int pgpu_batch_ct_conv2d_signed(const pgpu_pubkey* key, const pgpu_batch* x, const pgpu_batch* w, const pgpu_conv2d_shape* shape,
                                int e_bits, pgpu_batch** out);
int pgpu_batch_ct_spmv_signed(const pgpu_pubkey* key, const pgpu_batch* x, const uint64_t* row_ptr, const uint32_t* col_idx,
                              const pgpu_batch* w, size_t rows, int e_bits, pgpu_batch** out);
/* What the two signed calls would run (host-side queries, need no device; every output pointer may be NULL): the arguments
 * and fields of pgpu_ct_conv2d_plan / pgpu_ct_spmv_plan, with the window (and the tile) held against tables of 2^w + 1 rows
 * per element, table_bytes = elements of a pass (every column of x) * (2^w + 1) * row bytes, and products = the unsigned
 * count + 3 * (elements of x - 1) for the inversion.  PGPU_CONV_WINDOW / _TILE / _SLICES and PGPU_SPMV_WINDOW / _CHUNK force
 * the signed calls too, read at every call.  Errors as pgpu_ct_conv2d_plan / pgpu_ct_spmv_plan. */
int pgpu_ct_conv2d_signed_plan(int key_bits, const pgpu_conv2d_shape* shape, int e_bits, int* window, int* slices, size_t* tile,
                               size_t* table_bytes, size_t* products);
int pgpu_ct_spmv_signed_plan(int key_bits, size_t rows, size_t cols, size_t nnz, size_t longest_row, int e_bits,
                             int* window, int* chunk, int* levels, size_t* table_bytes, size_t* products);

/* ---- re-indexing of resident batches: gather, concat, slice ----
 * Between two calls on resident batches a caller picks rows, puts batches end to end or cuts a result into parts without
 * leaving the device: a minibatch drawn from a resident data set, K clients' uploads stacked for pgpu_batch_ct_segment_sum,
 * a layer's output split or permuted.  The calls take no key and preserve the domain: they move rows as BYTES, so they work
 * on any batch -- plain uploaded words of any width (plaintext and randomness batches with words = 1 included), Montgomery
 * words, pair rows -- and the result is what the sources are.  THERE IS NO CONVERSION INSIDE THESE CALLS: all sources of
 * one call share one layout -- the same words, the same domain and, for pair rows or Montgomery words, the same context
 * (modulus and form) -- and a call that mixes layouts is PGPU_ERR_INVALID_PARAM.  A caller who holds uploaded ciphertext
 * words beside pair rows passes the uploaded batch through any ciphertext operation first, or gathers before mixing.
 *
 * pgpu_batch_gather: out[i] = row idx[i] of the concatenation of xs[0 .. n_src), n_out rows.  The same handle may appear
 * twice (it is then two stretches of the concatenation); indices may repeat and come in any order; idx is HOST memory,
 * consumed before the call returns.  PGPU_GATHER_ONE as an index yields the value 1 in the batch's domain -- the integer
 * 1, R mod N, or the pair row of one that the key's pair form holds: a ciphertext there decrypts to 0 (zero padding for an
 * im2col, a missing value).  One launch of row_gather_kernel (kind PGPU_KERNEL_GATHER): a row is read by neighbouring
 * lanes in contiguous 16-byte pieces (8-byte where the row size is no multiple of 16), several rows in flight per
 * wavefront (pgpu_batch_gather_plan reports the shape).
 * pgpu_batch_concat: gather with the identity index, done as one stream-ordered device-to-device copy per source, with
 * no index list and no kernel.
 * pgpu_batch_slice: rows start, start + step, ..., count of them.  step == 1 is one copy; step > 1 takes the kernel (the
 * strided read of an [n_vec][cols] batch as a column: start = column, step = cols, count = n_vec).
 * The result is an ordinary immutable resident batch on the lane of xs[0] (of x); sources on other lanes are ordered in by
 * the events pgpu_batch_ct_add uses.  Sources may be destroyed as soon as the call returns.
 * PGPU_ERR_INVALID_PARAM: null or stale handles, a null out (or idx); n_src == 0 or above 65535; n_out == 0; an index at or
 * beyond the total count that is not the sentinel (the message names the first offending position); a source of 2^32 - 1
 * rows or more; step == 0; a slice that runs past the end; a layout mismatch.  PGPU_ERR_UNSUPPORTED: pools of more than one
 * GPU, as for the aggregation calls.  All refusals are decided on the host before any launch or copy and leave *out
 * untouched.  SIDE CHANNELS: these calls are not refused under pgpu_set_table_gather_policy(1) -- the address stream
 * depends on the caller's plaintext indices only, as for upload and download. */
#define PGPU_GATHER_ONE 0xFFFFFFFFFFFFFFFFull
int pgpu_batch_gather(const pgpu_batch* const* xs, size_t n_src, const uint64_t* idx /* HOST, [n_out] */, size_t n_out,
                      pgpu_batch** out);
int pgpu_batch_concat(const pgpu_batch* const* xs, size_t n_src, pgpu_batch** out);
int pgpu_batch_slice(const pgpu_batch* x, size_t start, size_t count, size_t step, pgpu_batch** out);
/* The launch shape of a gather of n_out rows of row_bytes bytes (host-side query, needs no device; every output pointer may
 * be NULL): lanes per row (a power of two, at most 16), rows per wavefront (64 / lanes, at least 4) and bytes per access
 * (16 where row_bytes % 16 == 0, else 8).  Row sizes: 8 * pgpu_batch_words, or 4 * pgpu_batch_row_limbs for pair rows (304,
 * 576, 896 bytes for 1024-, 2048-, 3072-bit keys).  PGPU_ERR_INVALID_PARAM: row_bytes == 0 or no multiple of 8, n_out == 0. */
int pgpu_batch_gather_plan(size_t row_bytes, size_t n_out, int* lanes_per_row, int* rows_per_wavefront, int* vec_bytes);

/* ---- instrumentation used by bench.py (roofline) ----
 * With timing enabled every kernel launch is bracketed by two HIP events recorded on the stream
 * the kernel is launched on (no synchronisation at launch time).  pgpu_timing_collect waits for
 * the recorded launches, writes up to max_entries (kind, milliseconds) pairs in launch order,
 * clears the record and returns the number written. */
typedef enum pgpu_kernel_kind {
  PGPU_KERNEL_MODEXP = 1,     /* modexp_kernel (generic / encrypt / decrypt stage 1) */
  PGPU_KERNEL_MODMUL = 2,     /* modmul_kernel */
  PGPU_KERNEL_CRT = 3,        /* crt_kernel (decrypt stage 2) */
  PGPU_KERNEL_FB_ENCRYPT = 4, /* fb_encrypt_kernel (DJN encrypt, fixed-base) */
  PGPU_KERNEL_MATVEC = 5,     /* every launch of pgpu_batch_ct_matvec: table build, multi-exponentiation, fold */
  PGPU_KERNEL_SEGSUM = 6,     /* every launch of pgpu_batch_ct_segment_sum: one per level */
  PGPU_KERNEL_SEGSCAN = 7,    /* every launch of pgpu_batch_ct_segment_scan: up-sweeps (segsum_kernel) and scans */
  PGPU_KERNEL_PACK = 8,       /* the launch of pgpu_batch_ct_pack */
  PGPU_KERNEL_SPMV = 9,       /* every launch of pgpu_batch_ct_spmv (and of _spmv_signed but its inversion): table build, multi-exponentiation, fold levels */
  PGPU_KERNEL_WSUM = 10,      /* every launch of pgpu_batch_ct_weighted_sum: the slices' schedules, the fold */
  PGPU_KERNEL_MATMUL = 11,    /* every launch of pgpu_batch_ct_matmul: per pass the table build, the multi-exponentiation, the fold */
  PGPU_KERNEL_BUCKET = 12,    /* every launch of pgpu_batch_ct_matvec_bucket: accumulation levels, bucket reductions, Horner */
  PGPU_KERNEL_CONV = 13,      /* every launch of pgpu_batch_ct_conv2d (and of _conv2d_signed but its inversion): per pass the table build, the multi-exponentiation, the fold */
  PGPU_KERNEL_INVERT = 14,    /* every launch of pgpu_batch_ct_negate / _sub: forward passes, walks back, the broadcast product */
  PGPU_KERNEL_GATHER = 15     /* row_gather_kernel: pgpu_batch_gather and the strided pgpu_batch_slice (form PGPU_FORM_FULL_WIDTH);
                                 pgpu_batch_concat and the unit-step slice are copies and record nothing */
} pgpu_kernel_kind;
int pgpu_set_timing(int enabled);
int pgpu_timing_collect(int* kinds, double* ms, int max_entries);
/* the same with the kernel FORM the launcher picked for each launch (forms may be NULL): bit 0 the paired split form
 * (hensel.hpp: the two halves of a residue in neighbouring lanes), bit 1 the sequential-halves form (hensel_seq.hpp:
 * both halves in the same lanes), bit 4 the launch claimed whole CUs (a half-chip launch beside a busy neighbour lane);
 * 0: a full-width kernel.  With the adaptive policy the form depends on what the GPU's other batch lanes were doing
 * at launch time, so a measurement reports what actually ran. */
typedef enum pgpu_kernel_form {
  PGPU_FORM_FULL_WIDTH = 0,
  PGPU_FORM_PAIRED = 1,
  PGPU_FORM_SEQ = 2,
  PGPU_FORM_LANE = 4,      /* a whole exponentiation per lane; always together with PGPU_FORM_PS since round 6 */
  PGPU_FORM_PS = 8,        /* with PGPU_FORM_LANE: by product scanning (hensel_ps.hpp: 1024- to 3072-bit keys; round 5) */
  PGPU_FORM_CU_CLAIM = 16,
  PGPU_FORM_WAVE = 32      /* one exponentiation per WAVEFRONT (hensel_wave.hpp, hensel_wave_n2.hpp: small launches of CRT decrypt, DJN
                              encrypt onto pair rows, CT x PT on pair rows; round 6) */
} pgpu_kernel_form;
int pgpu_timing_collect_ex(int* kinds, int* forms, double* ms, int max_entries);
/* ... and as a small kernel trace: batch lane of each launch (-1: another stream) and its start relative to the first
 * recorded launch, from the same HIP events (any of forms / lanes / start_ms may be NULL) */
int pgpu_timing_collect_trace(int* kinds, int* forms, int* lanes, double* start_ms, double* ms, int max_entries);
/* Kernel geometry a batch of `count` exponentiations / products under an odd modulus of mod_bits bits
 * (operand rows of in_words 64-bit words) is launched with: *lanes lanes per element, *limbs 29-bit limbs
 * per lane (modexp_kernel; small batches take a 16-lane latency split, large ones the wide split).  Pure
 * host-side query (needs no device); lets a profile be labelled with the kernel instantiation that ran.  PGPU_ERR_UNSUPPORTED when no compiled geometry is wide enough. */
int pgpu_kernel_geometry(int in_words, int mod_bits, size_t count, int* lanes, int* limbs);
/* Exponentiation kernel a CRT decrypt of `count` ciphertexts (per device) runs under this key: *split = 1:
 * hensel_decrypt_kernel<*lanes / 2, *limbs> -- residues modulo p^2 / q^2 as pairs of half-width numbers (DESIGN.md
 * section 3; compiled for 1024- to 4096-bit keys; PGPU_HENSEL=0 turns it off); *split = 2: for ciphertexts of a
 * resident batch (pair rows), hensel_decrypt_seq_kernel<*lanes, *limbs> -- both halves of a pair in the same *lanes
 * lanes, launches that still put a wavefront on every SIMD that way (PGPU_SEQ_DECRYPT=0 turns it off); (*split = 3 named
 * round 4's operand-scanning one-lane kernel, retired in round 6;) *split = 4 (round 5):
 * hensel_decrypt_ps_kernel<*limbs, 28 | 29> -- a whole exponentiation in one lane by product scanning, *limbs limbs per half
 * (38 / 56 limbs of 28 bits: 2048- / 3072-bit keys, 19 limbs of 29 bits: 1024-bit keys; launches of
 * more than 16384 ciphertexts (3072-bit keys: 24576) in rounds of 32768 -- the form reported is that of the full rounds; a
 * mostly empty last round runs as a launch of its own in the form of its size -- or smaller ones that cover the SIMDs
 * together with busy neighbour lanes: 8192 beside three;
 * PGPU_PS_DECRYPT=0 turns it off); *split = 5 (round 6): hensel_decrypt_wave_kernel<*limbs, 28 | 29> -- one exponentiation per
 * wavefront (*lanes = 64), a limb per lane: lone decrypts of up to 512 ciphertexts of 1024- to 3072-bit keys;
 * *split = 0: the full-width modexp_kernel<Geo<*lanes, *limbs>>.
 * Host-side query. */
int pgpu_decrypt_kernel_form(const pgpu_privkey* key, size_t count, int* split, int* lanes, int* limbs);
/* ... when `busy_lanes` OTHER batch lanes of the GPU have work queued at launch time (round 4, the adaptive policy: a
 * launch that will share the chip anyway takes the sequential-halves form as soon as waves * (1 + busy_lanes) covers the
 * SIMDs; pgpu_decrypt_kernel_form is the busy_lanes = 0 case, a lone caller) */
int pgpu_decrypt_kernel_form_ex(const pgpu_privkey* key, size_t count, int busy_lanes, int* split, int* lanes, int* limbs);
/* The same for an encrypt of `count` plaintext rows of m_words words: *split = 1: hensel_fb_encrypt_kernel<*lanes / 2,
 * *limbs> (DJN keys with a fixed-base window, 1024- to 3072-bit keys, plaintext rows no wider than n, batches that
 * fill the chip); *split = 2: results that stay resident as pair rows, launches that still put a wavefront on every SIMD
 * with half the lanes per element: hensel_fb_encrypt_seq_kernel<*lanes, *limbs> (PGPU_SEQ_DECRYPT=0 turns it off);
 * *split = 5 (round 6; asked for with busy_lanes = -1 through the _ex form: "the results stay resident as pair rows"): at most
 * 1024 elements: hensel_fb_encrypt_wave_kernel<*limbs, ...> -- one wavefront per element (*lanes = 64), *limbs limbs per half of the row; *split = 0: fb_encrypt_kernel / modexp_kernel
 * <Geo<*lanes, *limbs>>. */
int pgpu_encrypt_kernel_form(const pgpu_pubkey* key, int m_words, size_t count, int* split, int* lanes, int* limbs);
int pgpu_encrypt_kernel_form_ex(const pgpu_pubkey* key, int m_words, size_t count, int busy_lanes, int* split, int* lanes,
                                int* limbs);
/* The same for the exponentiations modulo n^2 with per-element bases (CT x PT of a resident batch, the non-DJN
 * obfuscator r^n): *split = 1: hensel_modexp_kernel<*lanes / 2, *limbs>; *split = 2: the same for r^n, and for CT x PT
 * of a resident batch (pair rows in and out, per-element exponents) hensel_modexp_seq_kernel<*lanes, *limbs> (both halves
 * of a pair in the same *lanes lanes; PGPU_SEQ_DECRYPT=0 turns it off); *split = 5 (round 6): CT x PT of at most 1024 resident
 * elements, hensel_modexp_wave_kernel<*limbs, ...> -- one wavefront per element; *split = 0: modexp_kernel<Geo<*lanes, *limbs>>. */
int pgpu_modexp_n2_kernel_form(const pgpu_pubkey* key, size_t count, int* split, int* lanes, int* limbs);
/* The same for CT + CT of two resident batches of `count` elements (per device): *split = 1: pair_ops_kernel<*lanes / 2,
 * *limbs> (one pair product on pair rows); *split = 2: pair_mul_seq_kernel<*lanes, *limbs> (both halves of a pair in the
 * same *lanes lanes: launches that still put a wavefront on every SIMD that way); *split = 0: modmul_kernel<Geo<*lanes,
 * *limbs>> on Montgomery-form words (keys without a pair form, PGPU_PAIR_ROWS=0). */
int pgpu_ct_add_kernel_form(const pgpu_pubkey* key, size_t count, int* split, int* lanes, int* limbs);

#ifdef __cplusplus
}
#endif

#endif /* PGPU_H_ */
