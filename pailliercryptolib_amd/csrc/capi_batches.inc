// pailliercryptolib_amd -- sharded device-resident batches (pgpu_batch_*): upload / download, the resident operations, batch lanes.
// Part of the translation unit of capi.cpp (included there, in place): the helpers of its anonymous namespaces --
// Montgomery contexts, geometry selection, launch wrappers -- are shared by every part.  Round 5 cut the file by topic;
// the kernel-form policy is a translation unit of its own (policy.cpp).

// ===================== sharded device-resident batches =====================
namespace {
// per-thread pinned bounce buffer for small uploads / downloads issued from the calling thread itself
constexpr size_t kBounceBytes = (size_t)256 << 10;
struct Bounce {
  void* p = nullptr;
  hipEvent_t ev = nullptr;
  bool pending = false;      // an upload still reads the buffer
  uint64_t gen = 0;
  int ready() {
    if (p && gen != rt::pool_generation()) {   // the pool this buffer's event belongs to is gone
      if (ev) (void)hipEventDestroy(ev);
      ev = nullptr;
      pending = false;
    }
    if (!p) HIP_TRY(hipHostMalloc(&p, kBounceBytes, hipHostMallocPortable));
    if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    gen = rt::pool_generation();
    if (pending) {
      HIP_TRY(hipEventSynchronize(ev));
      pending = false;
    }
    return PGPU_OK;
  }
  ~Bounce() {
    // (a thread that ends while the pool is up gives its buffer back; at process exit the HIP runtime may already be
    // shutting down, so nothing is touched then and the driver reclaims the memory)
    if (!rt::initialized() || gen != rt::pool_generation()) return;
    if (ev) (void)hipEventDestroy(ev);
    if (p) (void)hipHostFree(p);
  }
};
Bounce& bounce() {
  thread_local Bounce b;
  return b;
}
}  // namespace

int pgpu_batch_create(size_t count, int words, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!out) return fail(PGPU_ERR_INVALID_PARAM, "null output pointer");
  std::unique_ptr<pgpu_batch> b;
  RC_TRY(new_batch(count, words, &b));
  *out = b.release();
  return PGPU_OK;
}

void pgpu_batch_destroy(pgpu_batch* b) { delete b; }
size_t pgpu_batch_count(const pgpu_batch* b) { return b ? b->count : 0; }
int pgpu_batch_words(const pgpu_batch* b) { return b ? b->words : 0; }
int pgpu_batch_is_montgomery(const pgpu_batch* b) { return b && (b->mont || b->pair_l2) ? 1 : 0; }   // any device-side domain

int pgpu_batch_upload(const uint64_t* host, size_t count, int words, size_t stride, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  rt::note_caller();
  if (!host || !out) return fail(PGPU_ERR_INVALID_PARAM, "null pointer");
  if (words <= 0 || stride < (size_t)words) return fail(PGPU_ERR_INVALID_PARAM, "stride smaller than the row width");
  std::unique_ptr<pgpu_batch> b;
  RC_TRY(new_batch(count, words, &b));
  pgpu_batch* bp = b.get();
  if (stride == (size_t)words && rt::host_is_pinned(host, count * (size_t)words * 8)) {
    // a buffer from pgpu_host_alloc is the DMA source itself: one copy per shard, queued from the calling thread on the
    // batch lane, NOT waited for (pgpu_host_wait / pgpu_host_free do, include/pgpu.h)
    for (int d = 0; d < bp->ndev; ++d) {
      size_t lo, hi;
      bp->bounds(d, &lo, &hi);
      rt::Device& dev = rt::device(d);
      rt::DeviceGuard g(dev.ordinal);
      hipStream_t s = dev.bs(bp->lane);
      const uint64_t* src = host + lo * (size_t)words;
      const size_t bytes = (hi - lo) * (size_t)words * 8;
      HIP_TRY(hipMemcpyAsync(bp->ptr(d), src, bytes, hipMemcpyHostToDevice, s));
      rt::host_note_read(src, bytes, dev.index, s);
    }
    *out = b.release();
    return PGPU_OK;
  }
  if (bp->ndev == 1 && stride == (size_t)words && count * (size_t)words * 8 <= kBounceBytes) {
    // small transfer: through the calling thread's own pinned bounce buffer -- no hand-over to a worker lane (a thread
    // wake-up costs more than the copy: Add_CTCT(16) at the ipcl:: API is 60 us of which the GPU works 10)
    rt::Device& dev = rt::device(0);
    rt::DeviceGuard g(dev.ordinal);
    Bounce& bn = bounce();
    RC_TRY(bn.ready());
    const size_t bytes = count * (size_t)words * 8;
    std::memcpy(bn.p, host, bytes);
    hipStream_t s = dev.bs(bp->lane);
    HIP_TRY(hipMemcpyAsync(bp->ptr(0), bn.p, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(bn.ev, s));
    bn.pending = true;
    *out = b.release();
    return PGPU_OK;
  }
  rt::TaskGroup tg;
  for (int d = 0; d < bp->ndev; ++d) {
    tg.run(rt::device(d), [=](rt::Lane& lane) -> int {
      size_t lo, hi;
      bp->bounds(d, &lo, &hi);
      hipStream_t s = lane.dev->bs(bp->lane);
      if (stride == (size_t)words) {
        RC_TRY(lane.h2d(bp->ptr(d), host + lo * (size_t)words, (hi - lo) * (size_t)words * 8, s));
      } else {   // rows padded to a wider stride on the host: the device batch is dense
        std::vector<uint64_t> dense((hi - lo) * (size_t)words);
        for (size_t i = lo; i < hi; ++i)
          std::memcpy(dense.data() + (i - lo) * (size_t)words, host + i * stride, (size_t)words * 8);
        RC_TRY(lane.h2d(bp->ptr(d), dense.data(), dense.size() * 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return PGPU_OK;
      }
      HIP_TRY(hipStreamSynchronize(s));   // the caller may reuse `host` as soon as we return
      return PGPU_OK;
    });
  }
  RC_TRY(tg.wait());
  *out = b.release();
  return PGPU_OK;
}

namespace {
// one task per shard on the pool's worker lanes: conversion kernel (if any), then the copy -- which Lane::d2h hands to the
// copy engine only once the batch's kernels have run
void download_tasks(rt::TaskGroup& tg, const pgpu_batch* b, uint64_t* host, int nd, bool async = false) {
  for (int d = 0; d < nd; ++d) {
    tg.run(rt::device(d), [=](rt::Lane& lane) -> int {
      struct Force { bool on; Force(bool o) : on(o) { if (on) rt::force_presync(true); } ~Force() { if (on) rt::force_presync(false); } } force(async);
      size_t lo, hi;
      b->bounds(d, &lo, &hi);
      rt::Device& dev = *lane.dev;
      hipStream_t s = dev.bs(b->lane);
      const size_t bytes = (hi - lo) * (size_t)b->words * 8;
      if (b->pair_l2) {   // pair rows: the plain value materialises here
        rt::DevMem plain;
        RC_TRY(plain.alloc(dev, s, bytes));
        rt::DeviceGuard g(dev.ordinal);
        RC_TRY(pair_to_words_on(dev, b->pair_form.get(), b->prow(d), (uint64_t*)plain.p, hi - lo, s));
        return lane.d2h(host + lo * (size_t)b->words, plain.p, bytes, s);
      }
      if (!b->mont) return lane.d2h(host + lo * (size_t)b->words, b->ptr(d), bytes, s);
      rt::DevMem plain;   // leave the Montgomery domain on the way out
      RC_TRY(plain.alloc(dev, s, bytes));
      RC_TRY(modmul_on(dev, *b->mont, pgpu::MM_BY_ONE, b->ptr(d), nullptr, 0, 0, (uint64_t*)plain.p, hi - lo, s));
      return lane.d2h(host + lo * (size_t)b->words, plain.p, bytes, s);
    });
  }
}
}  // namespace

int pgpu_batch_download(const pgpu_batch* b, uint64_t* host) {
  RC_TRY(rt::check_ready());
  rt::note_caller();
  if (!b || !host) return fail(PGPU_ERR_INVALID_PARAM, "null pointer");
  RC_TRY(check_gen(b->gen, "batch"));
  const int nd = b->replicated ? 1 : b->ndev;
  if (rt::host_is_pinned(host, b->count * (size_t)b->words * 8)) {
    // pinned target (pgpu_host_alloc): conversion kernel (if any) and ONE DMA per shard, queued from the calling thread;
    // then the shards are waited for
    std::vector<rt::DevMem> plain((size_t)nd);
    for (int d = 0; d < nd; ++d) {
      size_t lo, hi;
      b->bounds(d, &lo, &hi);
      rt::Device& dev = rt::device(d);
      rt::DeviceGuard g(dev.ordinal);
      hipStream_t s = dev.bs(b->lane);
      const size_t bytes = (hi - lo) * (size_t)b->words * 8;
      const void* src = b->ptr(d);
      if (b->pair_l2 || b->mont) {
        RC_TRY(plain[(size_t)d].alloc(dev, s, bytes));
        if (b->pair_l2) RC_TRY(pair_to_words_on(dev, b->pair_form.get(), b->prow(d), (uint64_t*)plain[(size_t)d].p, hi - lo, s));
        else RC_TRY(modmul_on(dev, *b->mont, pgpu::MM_BY_ONE, b->ptr(d), nullptr, 0, 0, (uint64_t*)plain[(size_t)d].p, hi - lo, s));
        src = plain[(size_t)d].p;
      }
      HIP_TRY(rt::drain_before_copy(s));
      HIP_TRY(hipMemcpyAsync(host + lo * (size_t)b->words, src, bytes, hipMemcpyDeviceToHost, s));
    }
    for (int d = 0; d < nd; ++d) {
      rt::Device& dev = rt::device(d);
      rt::DeviceGuard g(dev.ordinal);
      hipError_t e = hipStreamSynchronize(dev.bs(b->lane));
      if (e != hipSuccess) return fail(PGPU_ERR_HIP, std::string("device -> host copy failed: ") + hipGetErrorString(e));
    }
    return PGPU_OK;
  }
  if (nd == 1 && b->count * (size_t)b->words * 8 <= kBounceBytes) {   // small transfer: the calling thread's bounce buffer
    rt::Device& dev = rt::device(0);
    rt::DeviceGuard g(dev.ordinal);
    Bounce& bn = bounce();
    RC_TRY(bn.ready());
    hipStream_t s = dev.bs(b->lane);
    const size_t bytes = b->count * (size_t)b->words * 8;
    rt::DevMem plain;
    const void* src = b->ptr(0);
    if (b->pair_l2 || b->mont) {
      RC_TRY(plain.alloc(dev, s, bytes));
      if (b->pair_l2) RC_TRY(pair_to_words_on(dev, b->pair_form.get(), b->prow(0), (uint64_t*)plain.p, b->count, s));
      else RC_TRY(modmul_on(dev, *b->mont, pgpu::MM_BY_ONE, b->ptr(0), nullptr, 0, 0, (uint64_t*)plain.p, b->count, s));
      src = plain.p;
    }
    HIP_TRY(rt::drain_before_copy(s));
    HIP_TRY(hipMemcpyAsync(bn.p, src, bytes, hipMemcpyDeviceToHost, s));
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(PGPU_ERR_HIP, std::string("device -> host copy failed: ") + hipGetErrorString(e));
    std::memcpy(host, bn.p, bytes);
    return PGPU_OK;
  }
  rt::TaskGroup tg;
  download_tasks(tg, b, host, nd);
  return tg.wait();
}

// Rows land `host_stride` words apart (host_stride >= words; the words in between are OVERWRITTEN WITH ZEROS: the rows
// travel as one linear copy of a device image whose gaps are cleared first -- a caller's own headers between the rows must
// be written after the call, and no stale device memory reaches the host): the ipcl:: layer lays
// results out as blocks of its limb allocator -- a 16-byte header in front of every row -- so that the BigNumbers point
// into the pinned block instead of copying out of it.  Pinned targets (pgpu_host_alloc) and one-GPU pools only; plain and
// pair-row batches (others: PGPU_ERR_UNSUPPORTED, the caller takes pgpu_batch_download).
int pgpu_batch_download_strided(const pgpu_batch* b, uint64_t* host, size_t host_stride) {
  RC_TRY(rt::check_ready());
  rt::note_caller();
  if (!b || !host) return fail(PGPU_ERR_INVALID_PARAM, "null pointer");
  RC_TRY(check_gen(b->gen, "batch"));
  if (host_stride < (size_t)b->words) return fail(PGPU_ERR_INVALID_PARAM, "download stride narrower than the rows");
  const size_t span = ((b->count - 1) * host_stride + (size_t)b->words) * 8;
  if ((b->replicated ? 1 : b->ndev) != 1 || (b->mont && !b->pair_l2) || !rt::host_is_pinned(host, span))
    return fail(PGPU_ERR_UNSUPPORTED, "strided download: pinned target, one GPU, plain or pair-row batch");
  rt::Device& dev = rt::device(0);
  rt::DeviceGuard g(dev.ordinal);
  hipStream_t s = dev.bs(b->lane);
  rt::DevMem tmp;
  RC_TRY(tmp.alloc(dev, s, span));
  if (host_stride > (size_t)b->words) HIP_TRY(hipMemsetAsync(tmp.p, 0, span, s));   // (the gaps: recycled device memory otherwise)
  if (b->pair_l2) {
    RC_TRY(pair_to_words_on(dev, b->pair_form.get(), b->prow(0), (uint64_t*)tmp.p, b->count, s, host_stride));
  } else {
    HIP_TRY(hipMemcpy2DAsync(tmp.p, host_stride * 8, b->ptr(0), (size_t)b->words * 8, (size_t)b->words * 8, b->count,
                             hipMemcpyDeviceToDevice, s));
  }
  HIP_TRY(rt::drain_before_copy(s));
  HIP_TRY(hipMemcpyAsync(host, tmp.p, span, hipMemcpyDeviceToHost, s));
  hipError_t e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(PGPU_ERR_HIP, std::string("device -> host copy failed: ") + hipGetErrorString(e));
  return PGPU_OK;
}

// ---- downloads that do not hold the caller ----
struct pgpu_ticket {
  rt::TaskGroup tg;
  uint64_t gen = 0;
};

int pgpu_batch_download_async(const pgpu_batch* b, uint64_t* host, pgpu_ticket** out) {
  RC_TRY(rt::check_ready());
  if (!b || !host || !out) return fail(PGPU_ERR_INVALID_PARAM, "null pointer");
  RC_TRY(check_gen(b->gen, "batch"));
  std::unique_ptr<pgpu_ticket> t(new pgpu_ticket);
  t->gen = b->gen;
  download_tasks(t->tg, b, host, b->replicated ? 1 : b->ndev, true);
  *out = t.release();
  return PGPU_OK;
}

int pgpu_ticket_wait(pgpu_ticket* t) {
  if (!t) return fail(PGPU_ERR_INVALID_PARAM, "null ticket");
  const int rc = t->tg.wait();
  delete t;
  return rc;
}

int pgpu_batch_encrypt(const pgpu_pubkey* key, const pgpu_batch* m, const pgpu_batch* r, int r_bits,
                       pgpu_batch** c) {
  RC_TRY(rt::check_ready());
  if (!key || !m || !r || !c) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(m->gen, "batch"));
  RC_TRY(check_gen(r->gen, "batch"));
  if (m->count != r->count) return fail(PGPU_ERR_INVALID_PARAM, "modExp: input vector size error");
  if (m->mont || r->mont) return fail(PGPU_ERR_INVALID_PARAM, "encrypt: operands must be plain batches");
  if (m->pair_l2 || r->pair_l2) return fail(PGPU_ERR_INVALID_PARAM, "encrypt: operands must be plain batches");
  RC_TRY(same_layout(m, r));
  // Keys with a split form keep their resident ciphertexts as PAIR ROWS (kargs.hpp) whenever the obfuscator runs
  // through a split-form kernel: DJN with a fixed-base table, or r^n.  Plaintext rows wider than n take the full-width
  // kernels and leave Montgomery-form words, as in round 2; consumers convert on the way in.
  const int l2 = (pair_form(key) && 64 * m->words <= key->n.BitSize() && (!key->djn || fixed_base_window() > 0) &&
                  (key->djn || r->words <= 2 * key->n_words))
                     ? pair_l2(key) : 0;
  std::unique_ptr<pgpu_batch> out;
  RC_TRY(new_batch(m->count, 2 * key->n_words, &out, l2, m->lane));
  if (l2) out->pair_form = pair_form_shared(key);
  else out->mont = key->nsq;
  for (int d = 0; d < out->ndev; ++d) {
    size_t lo, hi;
    out->bounds(d, &lo, &hi);
    rt::Device& dev = rt::device(d);
    rt::DeviceGuard g(dev.ordinal);
    RC_TRY(lane_acquire(dev, r, m->lane));
    RC_TRY(encrypt_on(dev, key, m->ptr(d), (size_t)m->words, m->words, r->ptr(d), (size_t)r->words, r->words, r_bits,
                      l2 ? nullptr : out->ptr(d), hi - lo, dev.bs(m->lane), true, m->count, l2 ? out->prow(d) : nullptr,
                      l2 ? busy_other_lanes(dev, m->lane, false, hi - lo) : 0));
    RC_TRY(lane_release(dev, r, m->lane));
  }
  if (key->djn) {
    std::lock_guard<std::mutex> lk(key->mu);
    key->fb_elems += m->count;
  }
  *c = out.release();
  return PGPU_OK;
}

int pgpu_batch_decrypt_crt(const pgpu_privkey* key, const pgpu_batch* c, pgpu_batch** m) {
  RC_TRY(rt::check_ready());
  if (!key || !c || !m) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(c->gen, "batch"));
  if (c->words != 2 * key->n_words) return fail(PGPU_ERR_INVALID_PARAM, "decrypt: ciphertext width mismatch");
  if (c->mont && c->mont->geo.rbits() != key->nsq_rbits)
    return fail(PGPU_ERR_INVALID_PARAM, "decrypt: ciphertext batch belongs to a different key size");
  // pair rows enter the split-form kernel as they are; when this launch would not take it (PGPU_HENSEL=0, a key class
  // without the form) they become plain words first
  std::unique_ptr<pgpu_batch> tmp;
  if (c->pair_l2) {
    size_t lo0, hi0;
    c->bounds(0, &lo0, &hi0);
    const pgpu_privkey::HenselSet* hset = pick_hensel(key, hi0 - lo0);
    if (!hset || hset->pair_l2 != c->pair_l2) {
      const pgpu_batch* cw = nullptr;
      RC_TRY(as_word_batch(c, &cw, &tmp));
      c = cw;
    }
  }
  std::unique_ptr<pgpu_batch> out;
  RC_TRY(new_batch(c->count, key->n_words, &out, 0, c->lane));
  for (int d = 0; d < out->ndev; ++d) {
    size_t lo, hi;
    out->bounds(d, &lo, &hi);
    rt::Device& dev = rt::device(d);
    rt::DeviceGuard g(dev.ordinal);
    if (c->pair_l2) {
      // are the GPU's other batch lanes busy right now?  Then this launch will share the chip with theirs
      const int busy = busy_other_lanes(dev, c->lane, false, hi - lo);
      RC_TRY(decrypt_on(dev, key, nullptr, out->ptr(d), hi - lo, dev.bs(c->lane), false, c->prow(d), c->pair_l2, busy));
    }
    else   // (word ciphertexts: decrypt_on converts them when the launch then takes a pair-row kernel)
      RC_TRY(decrypt_on(dev, key, c->ptr(d), out->ptr(d), hi - lo, dev.bs(c->lane), c->mont != nullptr, nullptr, 0,
                        busy_other_lanes(dev, c->lane, false, hi - lo)));
  }
  *m = out.release();
  return PGPU_OK;
}

// brings a plain ciphertext batch into the key's Montgomery domain (fresh batch), shard by shard
static int to_montgomery(const pgpu_pubkey* key, const pgpu_batch* a, std::unique_ptr<pgpu_batch>* out) {
  std::unique_ptr<pgpu_batch> t;
  RC_TRY(new_batch(a->count, a->words, &t, 0, a->lane));
  t->mont = key->nsq;
  for (int d = 0; d < t->ndev; ++d) {
    size_t lo, hi;
    t->bounds(d, &lo, &hi);
    rt::Device& dev = rt::device(d);
    rt::DeviceGuard g(dev.ordinal);
    RC_TRY(modmul_on(dev, *key->nsq, pgpu::MM_BY_R2, a->ptr(d), nullptr, 0, 0, t->ptr(d), hi - lo, dev.bs(a->lane)));
  }
  *out = std::move(t);
  return PGPU_OK;
}

int pgpu_batch_ct_add(const pgpu_pubkey* key, const pgpu_batch* a, const pgpu_batch* b, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !a || !b || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(a->gen, "batch"));
  RC_TRY(check_gen(b->gen, "batch"));
  const int W = 2 * key->n_words;
  if (a->words != W || b->words != W) return fail(PGPU_ERR_INVALID_PARAM, "CT + CT error: width mismatch");
  if (b->count != a->count && b->count != 1) return fail(PGPU_ERR_INVALID_PARAM, "CT + CT error: Size mismatch!");
  if (!same_domain(a->mont, key->nsq) || !same_domain(b->mont, key->nsq))
    return fail(PGPU_ERR_INVALID_PARAM, "CT + CT error: 2 different public keys detected!");
  RC_TRY(same_layout(a, b));
  std::unique_ptr<pgpu_batch> ta, tb;
  if (const pgpu_pubkey::PubForm* f = pair_form(key)) {
    // pair rows: ONE pair product per element (5 instead of 8 s^2 limb products, no word <-> limb conversion)
    RC_TRY(as_pair_batch(key, a, &a, &ta));
    RC_TRY(as_pair_batch(key, b, &b, &tb));
    const int l2 = f->H * f->K;
    std::unique_ptr<pgpu_batch> o;
    RC_TRY(new_batch(a->count, W, &o, l2, a->lane));
    o->pair_form = pair_form_shared(key);
    RC_TRY(lanes_order(b, a->lane, true));
  const bool bcast = b->count == 1 && a->count != 1;
    for (int d = 0; d < o->ndev; ++d) {
      size_t lo, hi;
      o->bounds(d, &lo, &hi);
      rt::Device& dev = rt::device(d);
      rt::DeviceGuard g(dev.ordinal);
      pgpu::PairOpsArgs pa{};
      const pgpu_pubkey::PubForm* lf = pair_op_form(key, f, hi - lo);
      pa.ctx = hensel_pub_view(lf, dev.index);
      pa.op = pgpu::PO_MUL;
      pa.a = a->prow(d);
      pa.b = b->prow(b->replicated ? d : (bcast ? 0 : d));
      pa.b_stride = bcast ? 0 : (size_t)2 * l2;
      pa.out = o->prow(d);
      pa.count = hi - lo;
      RC_TRY(pair_op_launch(dev, lf, pa, dev.bs(a->lane), PGPU_KERNEL_MODMUL));
    }
    RC_TRY(lanes_order(b, a->lane, false));
    *out = o.release();
    return PGPU_OK;
  }
  if (a->pair_l2 || b->pair_l2) return fail(PGPU_ERR_INVALID_PARAM, "CT + CT error: 2 different public keys detected!");
  // both operands in the Montgomery domain -> ONE product per element, result stays there
  if (!a->mont) {
    RC_TRY(to_montgomery(key, a, &ta));
    a = ta.get();
  }
  if (!b->mont) {
    RC_TRY(to_montgomery(key, b, &tb));
    b = tb.get();
  }
  std::unique_ptr<pgpu_batch> o;
  RC_TRY(new_batch(a->count, W, &o, 0, a->lane));
  o->mont = key->nsq;
  RC_TRY(lanes_order(b, a->lane, true));
  const bool bcast = b->count == 1 && a->count != 1;
  for (int d = 0; d < o->ndev; ++d) {
    size_t lo, hi;
    o->bounds(d, &lo, &hi);
    rt::Device& dev = rt::device(d);
    rt::DeviceGuard g(dev.ordinal);
    RC_TRY(modmul_on(dev, *key->nsq, pgpu::MM_SINGLE, a->ptr(d), b->ptr(b->replicated ? d : (bcast ? 0 : d)),
                     bcast ? 0 : (size_t)W, 0, o->ptr(d), hi - lo, dev.bs(a->lane)));
  }
  RC_TRY(lanes_order(b, a->lane, false));
  *out = o.release();
  return PGPU_OK;
}

int pgpu_batch_ct_add_plain(const pgpu_pubkey* key, const pgpu_batch* a, const pgpu_batch* m, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !a || !m || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(a->gen, "batch"));
  RC_TRY(check_gen(m->gen, "batch"));
  const int W = 2 * key->n_words;
  if (a->words != W || m->words > W) return fail(PGPU_ERR_INVALID_PARAM, "CT + PT error: width mismatch");
  if (m->count != a->count && m->count != 1) return fail(PGPU_ERR_INVALID_PARAM, "CT + PT error: Size mismatch!");
  if (!same_domain(a->mont, key->nsq)) return fail(PGPU_ERR_INVALID_PARAM, "CT + PT error: batch belongs to a different key");
  if (m->mont || m->pair_l2) return fail(PGPU_ERR_INVALID_PARAM, "CT + PT error: plaintext batch in Montgomery form");
  RC_TRY(same_layout(a, m));
  std::unique_ptr<pgpu_batch> ta;
  const pgpu_pubkey::PubForm* pf = pair_form(key);
  if (pf && 64 * m->words <= key->n.BitSize()) {
    // pair rows: c * (1 + n*m) only changes the b half -- two half-width products (hensel.hpp: pair_times_gm)
    RC_TRY(as_pair_batch(key, a, &a, &ta));
    const int l2 = pf->H * pf->K;
    std::unique_ptr<pgpu_batch> o;
    RC_TRY(new_batch(a->count, W, &o, l2, a->lane));
    o->pair_form = pair_form_shared(key);
    RC_TRY(lanes_order(m, a->lane, true));
  const bool bcast = m->count == 1 && a->count != 1;
    for (int d = 0; d < o->ndev; ++d) {
      size_t lo, hi;
      o->bounds(d, &lo, &hi);
      rt::Device& dev = rt::device(d);
      rt::DeviceGuard g(dev.ordinal);
      pgpu::PairOpsArgs pa{};
      const pgpu_pubkey::PubForm* lf = pair_op_form(key, pf, hi - lo);
      pa.ctx = hensel_pub_view(lf, dev.index);
      pa.op = pgpu::PO_TIMES_GM;
      pa.a = a->prow(d);
      pa.words = m->ptr(m->replicated ? d : (bcast ? 0 : d));
      pa.words_stride = bcast ? 0 : (size_t)m->words;
      pa.nwords = m->words;
      pa.out = o->prow(d);
      pa.count = hi - lo;
      RC_TRY(pair_op_launch(dev, lf, pa, dev.bs(a->lane), PGPU_KERNEL_MODMUL));
    }
    RC_TRY(lanes_order(m, a->lane, false));
    *out = o.release();
    return PGPU_OK;
  }
  if (a->pair_l2) {   // plaintext rows wider than n: the full-width kernel, on plain words
    const pgpu_batch* aw = nullptr;
    RC_TRY(as_word_batch(a, &aw, &ta));
    a = aw;
  }
  std::unique_ptr<pgpu_batch> o;
  RC_TRY(new_batch(a->count, W, &o, 0, a->lane));
  o->mont = a->mont ? key->nsq : nullptr;   // the product keeps the form of the ciphertext
  RC_TRY(lanes_order(m, a->lane, true));
  const bool bcast = m->count == 1 && a->count != 1;
  for (int d = 0; d < o->ndev; ++d) {
    size_t lo, hi;
    o->bounds(d, &lo, &hi);
    rt::Device& dev = rt::device(d);
    rt::DeviceGuard g(dev.ordinal);
    RC_TRY(modmul_on(dev, *key->nsq, pgpu::MM_GM, a->ptr(d), m->ptr(m->replicated ? d : (bcast ? 0 : d)),
                     bcast ? 0 : (size_t)m->words, m->words, o->ptr(d), hi - lo, dev.bs(a->lane), VF_GM_MONT));
  }
  RC_TRY(lanes_order(m, a->lane, false));
  *out = o.release();
  return PGPU_OK;
}

int pgpu_batch_ct_mul(const pgpu_pubkey* key, const pgpu_batch* a, const pgpu_batch* e, int e_bits,
                      pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !a || !e || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(a->gen, "batch"));
  RC_TRY(check_gen(e->gen, "batch"));
  const int W = 2 * key->n_words;
  if (a->words != W) return fail(PGPU_ERR_INVALID_PARAM, "CT * PT error: width mismatch");
  if (e->count != a->count && e->count != 1) return fail(PGPU_ERR_INVALID_PARAM, "CT * PT error: Size mismatch!");
  if (e->mont) return fail(PGPU_ERR_INVALID_PARAM, "CT * PT error: exponent batch in Montgomery form");
  if (!same_domain(a->mont, key->nsq)) return fail(PGPU_ERR_INVALID_PARAM, "CT * PT error: batch belongs to a different key");
  if (e_bits < 0 || e_bits > 64 * e->words) return fail(PGPU_ERR_INVALID_PARAM, "exp_bits/exp_words inconsistent");
  if (e->pair_l2) return fail(PGPU_ERR_INVALID_PARAM, "CT * PT error: exponent batch in Montgomery form");
  RC_TRY(same_layout(a, e));
  RC_TRY(lanes_order(e, a->lane, true));
  const bool bcast = e->count == 1 && a->count != 1;
  std::unique_ptr<pgpu_batch> ta;
  if (const pgpu_pubkey::PubForm* pf = pair_form(key)) {
    // pair rows in, pair rows out: the split-form kernel starts from the row as it is and stores its result as it is.
    // Forms of the same limb count share the rows (2048-bit keys: (8,9) for small batches, (4,18) beyond).
    const int l2 = pf->H * pf->K;
    RC_TRY(as_pair_batch(key, a, &a, &ta));
    std::unique_ptr<pgpu_batch> o;
    RC_TRY(new_batch(a->count, W, &o, l2, a->lane));
    o->pair_form = pair_form_shared(key);
    for (int d = 0; d < o->ndev; ++d) {
      size_t lo, hi;
      o->bounds(d, &lo, &hi);
      rt::Device& dev = rt::device(d);
      rt::DeviceGuard g(dev.ordinal);
      const pgpu_pubkey::PubForm* form = split_modexp_form(key, hi - lo);
      if (!form || form->H * form->K != l2) form = pf;
      if (!pgpu::hensel_modexp_has(form->H, form->K)) return fail(PGPU_ERR_UNSUPPORTED, "split-form modexp kernel not compiled");
      RC_TRY(modexp_split_on(dev, key, form, nullptr, 0, W, false, e->ptr(e->replicated ? d : (bcast ? 0 : d)),
                             bcast ? 0 : (size_t)e->words, e->words, e_bits, nullptr, pgpu::FM_UNIT, nullptr, 0, 0, nullptr,
                             false, hi - lo, dev.bs(a->lane), a->prow(d), (size_t)2 * l2, o->prow(d)));
    }
    RC_TRY(lanes_order(e, a->lane, false));
    *out = o.release();
    return PGPU_OK;
  }
  if (a->pair_l2) return fail(PGPU_ERR_INVALID_PARAM, "CT * PT error: batch belongs to a different key");
  std::unique_ptr<pgpu_batch> o;
  RC_TRY(new_batch(a->count, W, &o, 0, a->lane));
  o->mont = key->nsq;
  std::vector<uint64_t> mod((size_t)W);
  key->nsq->N.toLimbs64(mod.data(), mod.size());
  for (int d = 0; d < o->ndev; ++d) {
    size_t lo, hi;
    o->bounds(d, &lo, &hi);
    rt::Device& dev = rt::device(d);
    rt::DeviceGuard g(dev.ordinal);
    if (const pgpu_pubkey::PubForm* form = split_modexp_form(key, hi - lo)) {
      RC_TRY(modexp_split_on(dev, key, form, a->ptr(d), (size_t)W, W, a->mont != nullptr,
                             e->ptr(e->replicated ? d : (bcast ? 0 : d)), bcast ? 0 : (size_t)e->words, e->words, e_bits,
                             nullptr, pgpu::FM_UNIT, nullptr, 0, 0, o->ptr(d), true, hi - lo, dev.bs(a->lane)));
      continue;
    }
    RC_TRY(modexp_on(dev, a->ptr(d), (size_t)W, e->ptr(e->replicated ? d : (bcast ? 0 : d)),
                     bcast ? 0 : (size_t)e->words, e->words, e_bits, mod.data(), W, o->ptr(d), hi - lo, dev.bs(a->lane),
                     nullptr, a->mont != nullptr, true, key->nsq));
  }
  RC_TRY(lanes_order(e, a->lane, false));
  *out = o.release();
  return PGPU_OK;
}

// ---- encrypted matrix-vector product (hensel_matvec.hpp; policy.hpp: matvec_*) ----
int pgpu_ct_matvec_plan(int key_bits, size_t rows, size_t cols, int e_bits, int* window, int* slices, size_t* table_bytes) {
  if (key_bits < 1 || rows == 0 || cols == 0 || e_bits < 1)
    return fail(PGPU_ERR_INVALID_PARAM, "matvec plan: key_bits, rows, cols and e_bits must be positive");
  int G = 0, K = 0;
  if (!policy::matvec_geometry(key_bits, &G, &K))
    return fail(PGPU_ERR_UNSUPPORTED, "matvec: keys of this size have no pair rows (1024- to 3072-bit key classes only)");
  const size_t row_bytes = (size_t)2 * G * K * sizeof(uint32_t);
  const size_t S = policy::matvec_slices(G, rows, cols);
  const int w = policy::matvec_window(rows, cols, e_bits, S, row_bytes);
  if (window) *window = w;
  if (slices) *slices = (int)S;
  if (table_bytes) *table_bytes = cols * ((size_t)1 << w) * row_bytes;
  return PGPU_OK;
}

int pgpu_batch_ct_matvec(const pgpu_pubkey* key, const pgpu_batch* x, const pgpu_batch* w, size_t rows, int e_bits,
                         pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !x || !w || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(x->gen, "batch"));
  RC_TRY(check_gen(w->gen, "batch"));
  const int W = 2 * key->n_words;
  const size_t cols = x->count;
  if (rows == 0) return fail(PGPU_ERR_INVALID_PARAM, "matvec error: rows must be positive");
  if (x->words != W) return fail(PGPU_ERR_INVALID_PARAM, "matvec error: ciphertext width mismatch");
  if (w->mont || w->pair_l2) return fail(PGPU_ERR_INVALID_PARAM, "matvec error: the matrix must be a plain uploaded batch");
  if (rows > ~(size_t)0 / cols || w->count != rows * cols)
    return fail(PGPU_ERR_INVALID_PARAM, "matvec error: Size mismatch! (the matrix must hold rows * count(x) values)");
  if (e_bits < 1 || e_bits > 64 * w->words) return fail(PGPU_ERR_INVALID_PARAM, "matvec error: e_bits outside the rows of the matrix batch");
  if (!same_domain(x->mont, key->nsq)) return fail(PGPU_ERR_INVALID_PARAM, "matvec error: batch belongs to a different key");
  if (rt::pool_size() > 1)
    return fail(PGPU_ERR_UNSUPPORTED, "matvec: pools of more than one GPU are not supported (rows are not sharded yet)");
  const pgpu_pubkey::PubForm* pf = pair_form(key);
  if (!pf || !pgpu::matvec_has(pf->H, pf->K))
    return fail(PGPU_ERR_UNSUPPORTED, "matvec: key has no pair form (1024- to 3072-bit keys; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0 switch it off)");
  // the window tables are addressed by digits of the caller's plaintext matrix: indexed access.  Under the masked
  // policy the call is refused rather than quietly breaking that promise.
  if (g_ct_gather.load())
    return fail(PGPU_ERR_UNSUPPORTED, "matvec: the masked table-gather policy is on (pgpu_set_table_gather_policy / PGPU_CT_GATHER) and "
                                      "this call indexes its window tables by digits of the plaintext matrix; no masked variant exists");
  std::unique_ptr<pgpu_batch> tx;
  RC_TRY(as_pair_batch(key, x, &x, &tx));
  const int G = pf->H, K = pf->K, l2 = G * K;
  const size_t LQ = (size_t)2 * l2, row_bytes = LQ * sizeof(uint32_t);
  const size_t S = policy::matvec_slices(G, rows, cols);
  const int win = policy::matvec_window(rows, cols, e_bits, S, row_bytes);
  std::unique_ptr<pgpu_batch> o;
  RC_TRY(new_batch(rows, W, &o, l2, x->lane));
  o->pair_form = pair_form_shared(key);
  rt::Device& dev = rt::device(0);
  rt::DeviceGuard g(dev.ordinal);
  hipStream_t s = dev.bs(x->lane);
  RC_TRY(lanes_order(w, x->lane, true));
  // table and partial products: the block arena, on the lane's stream like the operands themselves
  rt::DevMem table, partial;
  RC_TRY(table.alloc(dev, s, cols * ((size_t)1 << win) * row_bytes));
  if (S > 1) RC_TRY(partial.alloc(dev, s, S * rows * row_bytes));
  pgpu::MatvecArgs a{};
  a.ctx = hensel_pub_view(pf, dev.index);
  a.x = x->prow(0);
  a.table = (uint32_t*)table.p;
  a.w = w->ptr(0);
  a.w_stride = (size_t)w->words;
  a.w_words = w->words;
  a.e_bits = e_bits;
  a.window = win;
  a.slices = (int)S;
  a.rows = rows;
  a.cols = cols;
  a.out = S > 1 ? (uint32_t*)partial.p : o->prow(0);
  const size_t ipw = 64 / (size_t)G;
  auto blocks_of = [](size_t waves) { return (unsigned)((waves + pgpu::kWavesPerWG - 1) / pgpu::kWavesPerWG); };
  {
    TimerScope t(dev, s, PGPU_KERNEL_MATVEC, PGPU_FORM_SEQ);
    if (!pgpu::launch_matvec_table(G, K, a, blocks_of((cols + ipw - 1) / ipw), s))
      return fail(PGPU_ERR_UNSUPPORTED, "matvec kernels not compiled for this key class");
    HIP_TRY(hipGetLastError());
    t.stop();
  }
  {
    TimerScope t(dev, s, PGPU_KERNEL_MATVEC, PGPU_FORM_SEQ);
    if (!pgpu::launch_matvec(G, K, a, blocks_of(S * ((rows + ipw - 1) / ipw)), s))
      return fail(PGPU_ERR_UNSUPPORTED, "matvec kernels not compiled for this key class");
    HIP_TRY(hipGetLastError());
    t.stop();
  }
  // fold the S partial products of every row: ceil(log2 S) element-wise pair products over the slices, in place (slice h + k
  // into slice k; a group reads its two rows before it writes one), the last one into the result batch
  for (size_t cur = S; cur > 1;) {
    const size_t h = (cur + 1) / 2;
    pgpu::PairOpsArgs pa{};
    pa.count = (cur - h) * rows;
    const pgpu_pubkey::PubForm* lf = pair_op_form(key, pf, pa.count);
    pa.ctx = hensel_pub_view(lf, dev.index);
    pa.op = pgpu::PO_MUL;
    pa.a = (const uint32_t*)partial.p;
    pa.b = (const uint32_t*)partial.p + h * rows * LQ;
    pa.b_stride = LQ;
    pa.out = h == 1 ? o->prow(0) : (uint32_t*)partial.p;
    RC_TRY(pair_op_launch(dev, lf, pa, s, PGPU_KERNEL_MATVEC));
    cur = h;
  }
  RC_TRY(lanes_order(w, x->lane, false));
  *out = o.release();
  return PGPU_OK;
}

// ---- encrypted segmented sum (hensel_segsum.hpp; policy.hpp: segsum_*) ----
int pgpu_ct_segment_sum_plan(int key_bits, size_t elements, size_t segments, size_t longest_segment, int* chunk, int* levels) {
  if (key_bits < 1 || segments == 0 || longest_segment > elements)
    return fail(PGPU_ERR_INVALID_PARAM, "segment sum plan: key_bits and segments must be positive, longest_segment at most elements");
  int G = 0, K = 0;
  if (!policy::matvec_geometry(key_bits, &G, &K))
    return fail(PGPU_ERR_UNSUPPORTED, "segment sum: keys of this size have no pair rows (1024- to 3072-bit key classes only)");
  const int c = policy::segsum_chunk(G, elements);
  if (chunk) *chunk = c;
  if (levels) *levels = policy::segsum_levels(c, longest_segment);
  return PGPU_OK;
}

int pgpu_batch_ct_segment_sum(const pgpu_pubkey* key, const pgpu_batch* x, const uint32_t* ids, size_t groups,
                              size_t n_segments, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !x || !ids || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(x->gen, "batch"));
  const int W = 2 * key->n_words;
  const size_t cols = x->count;
  if (groups == 0 || n_segments == 0) return fail(PGPU_ERR_INVALID_PARAM, "segment sum error: groups and n_segments must be positive");
  if (x->words != W) return fail(PGPU_ERR_INVALID_PARAM, "segment sum error: ciphertext width mismatch");
  // (element numbers are 32-bit entries of the sorted list, segment and partial-row numbers 31-bit fields of a descriptor)
  constexpr size_t kMax = (size_t)1 << 31;
  if (cols >= kMax || groups >= kMax / cols || n_segments >= kMax / groups)
    return fail(PGPU_ERR_INVALID_PARAM, "segment sum error: groups * count(x) and groups * n_segments must stay below 2^31");
  if (!same_domain(x->mont, key->nsq)) return fail(PGPU_ERR_INVALID_PARAM, "segment sum error: batch belongs to a different key");
  if (rt::pool_size() > 1)
    return fail(PGPU_ERR_UNSUPPORTED, "segment sum: pools of more than one GPU are not supported (segments are not sharded yet)");
  const pgpu_pubkey::PubForm* pf = pair_form(key);
  if (!pf || !pgpu::matvec_has(pf->H, pf->K))
    return fail(PGPU_ERR_UNSUPPORTED, "segment sum: key has no pair form (1024- to 3072-bit keys; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0 switch it off)");
  // the rows of x are addressed by the caller's plaintext ids: indexed access.  Under the masked policy the call is refused
  // rather than quietly breaking that promise.
  if (g_ct_gather.load())
    return fail(PGPU_ERR_UNSUPPORTED, "segment sum: the masked table-gather policy is on (pgpu_set_table_gather_policy / PGPU_CT_GATHER) and "
                                      "this call addresses the ciphertext rows by the plaintext segment ids; no masked variant exists");
  if (x->pair_l2 && (x->pair_l2 != pf->H * pf->K || !(x->pair_form->n == key->n)))
    return fail(PGPU_ERR_INVALID_PARAM, "segment sum error: batch belongs to a different key");
  // the plan, on the host: sorted element numbers, chunk descriptors level by level
  const int G = pf->H, K = pf->K, l2 = G * K;
  const size_t LQ = (size_t)2 * l2, row_bytes = LQ * sizeof(uint32_t), segments = groups * n_segments;
  std::vector<uint32_t> perm;
  std::vector<size_t> offsets;
  if (!policy::segsum_sort(ids, groups, cols, n_segments, &perm, &offsets))
    return fail(PGPU_ERR_INVALID_PARAM, "segment sum error: a segment id is neither below n_segments nor PGPU_SEGMENT_NONE");
  policy::SegsumPlan plan;
  policy::segsum_plan(offsets, policy::segsum_chunk(G, perm.size()), &plan);
  // one image for the device: the sorted list (never empty: the kernel reads entry 0 for the groups past their end), then
  // the descriptors of every level
  const size_t perm_bytes = (std::max<size_t>(1, perm.size()) * sizeof(uint32_t) + 15) & ~(size_t)15;
  // partial rows: level l reads what level l - 1 wrote, so two regions serve all levels in turn
  size_t image_bytes = perm_bytes, region[2] = {0, 0};
  for (size_t l = 0; l < plan.levels.size(); ++l) {
    image_bytes += plan.levels[l].chunks.size() * sizeof(pgpu::SegsumChunk);
    region[l & 1] = std::max(region[l & 1], plan.levels[l].partial_rows);
  }
  std::vector<char> image(image_bytes, 0);
  if (!perm.empty()) std::memcpy(image.data(), perm.data(), perm.size() * sizeof(uint32_t));
  {
    size_t at = perm_bytes;
    for (const auto& lv : plan.levels) {
      std::memcpy(image.data() + at, lv.chunks.data(), lv.chunks.size() * sizeof(pgpu::SegsumChunk));
      at += lv.chunks.size() * sizeof(pgpu::SegsumChunk);
    }
  }
  std::unique_ptr<pgpu_batch> tx;
  RC_TRY(as_pair_batch(key, x, &x, &tx));
  std::unique_ptr<pgpu_batch> o;
  RC_TRY(new_batch(segments, W, &o, l2, x->lane));
  o->pair_form = pair_form_shared(key);
  rt::Device& dev = rt::device(0);
  rt::DeviceGuard g(dev.ordinal);
  hipStream_t s = dev.bs(x->lane);
  // plan image and partial rows: the block arena, on the lane's stream like the operands themselves -- what the arena hands
  // out again it hands to this stream, behind the kernels below
  rt::DevMem dimage, partial;
  RC_TRY(dimage.alloc(dev, s, image_bytes));
  if (region[0]) RC_TRY(partial.alloc(dev, s, (region[0] + region[1]) * row_bytes));
  if (image_bytes <= kBounceBytes) {
    Bounce& bn = bounce();
    RC_TRY(bn.ready());
    std::memcpy(bn.p, image.data(), image_bytes);
    HIP_TRY(hipMemcpyAsync(dimage.p, bn.p, image_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(bn.ev, s));
    bn.pending = true;
  } else {   // through a worker lane's staging buffers, queued on the same stream: nothing is waited for
    rt::TaskGroup tg;
    void* dst = dimage.p;
    const char* src = image.data();
    tg.run(dev, [=](rt::Lane& lane) -> int { return lane.h2d(dst, src, image_bytes, s); });
    RC_TRY(tg.wait());
  }
  // the form with the same limbs per half on more lanes, for the levels that leave SIMDs empty (2048-bit keys: (8,9))
  const pgpu_pubkey::PubForm* wide = nullptr;
  for (const auto& alt : key->hforms)
    if (alt->H * alt->K == l2 && alt->H > G && pgpu::segsum_wide_has(alt->H, alt->K)) wide = alt.get();
  pgpu::SegsumArgs a{};
  a.out = o->prow(0);
  uint32_t* const reg[2] = {(uint32_t*)partial.p, partial.p ? (uint32_t*)partial.p + region[0] * LQ : nullptr};
  size_t at = perm_bytes;
  for (size_t l = 0; l < plan.levels.size(); ++l) {
    const auto& lv = plan.levels[l];
    const pgpu_pubkey::PubForm* lf = wide && policy::segsum_wide_pays(wide->H, lv.chunks.size()) ? wide : pf;
    a.ctx = hensel_pub_view(lf, dev.index);
    a.src = l == 0 ? x->prow(0) : reg[(l - 1) & 1];
    a.perm = l == 0 ? (const uint32_t*)dimage.p : nullptr;
    a.chunks = (const pgpu::SegsumChunk*)((const char*)dimage.p + at);
    a.n_chunks = lv.chunks.size();
    a.partial = reg[l & 1];
    const size_t ipw = 64 / (size_t)lf->H, waves = (a.n_chunks + ipw - 1) / ipw;
    TimerScope t(dev, s, PGPU_KERNEL_SEGSUM, PGPU_FORM_SEQ);
    if (!pgpu::launch_segsum(lf->H, lf->K, a, (unsigned)((waves + pgpu::kWavesPerWG - 1) / pgpu::kWavesPerWG), s))
      return fail(PGPU_ERR_UNSUPPORTED, "segment sum kernels not compiled for this key class");
    HIP_TRY(hipGetLastError());
    t.stop();
    at += lv.chunks.size() * sizeof(pgpu::SegsumChunk);
  }
  *out = o.release();
  return PGPU_OK;
}

// ---- encrypted sparse matrix-vector product (hensel_spmv.hpp; policy.hpp: spmv_*) ----
int pgpu_ct_spmv_plan(int key_bits, size_t rows, size_t cols, size_t nnz, size_t longest_row, int e_bits,
                      int* window, int* chunk, int* levels, size_t* table_bytes, size_t* products) {
  constexpr size_t kMax = (size_t)1 << 31;
  if (key_bits < 1 || rows == 0 || cols == 0 || nnz == 0 || e_bits < 1 || longest_row == 0 || longest_row > nnz ||
      rows >= kMax || nnz >= kMax || (nnz + longest_row - 1) / longest_row > rows)
    return fail(PGPU_ERR_INVALID_PARAM, "spmv plan: key_bits, rows, cols, nnz and e_bits must be positive, rows and nnz below 2^31, "
                                        "longest_row between ceil(nnz / rows) and nnz");
  int G = 0, K = 0;
  if (!policy::matvec_geometry(key_bits, &G, &K))
    return fail(PGPU_ERR_UNSUPPORTED, "spmv: keys of this size have no pair rows (1024- to 3072-bit key classes only)");
  const size_t row_bytes = (size_t)2 * G * K * sizeof(uint32_t);
  const int c = policy::spmv_chunk(G, nnz, rows);
  const size_t chains = policy::spmv_chains_estimate(rows, nnz, longest_row, c);
  const int w = policy::spmv_window(rows, cols, nnz, chains, e_bits, row_bytes);
  if (window) *window = w;
  if (chunk) *chunk = c;
  if (levels) *levels = policy::spmv_levels(c, longest_row);
  if (table_bytes) *table_bytes = cols * ((size_t)1 << w) * row_bytes;
  if (products) *products = (size_t)policy::spmv_products(rows, cols, nnz, chains, e_bits, w);
  return PGPU_OK;
}

int pgpu_batch_ct_spmv(const pgpu_pubkey* key, const pgpu_batch* x, const uint64_t* row_ptr, const uint32_t* col_idx,
                       const pgpu_batch* w, size_t rows, int e_bits, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !x || !row_ptr || !col_idx || !w || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(x->gen, "batch"));
  RC_TRY(check_gen(w->gen, "batch"));
  const int W = 2 * key->n_words;
  const size_t cols = x->count;
  // (CSR positions, rows and chains are 31-bit fields of a descriptor)
  constexpr size_t kMax = (size_t)1 << 31;
  if (rows == 0 || rows >= kMax) return fail(PGPU_ERR_INVALID_PARAM, "spmv error: rows must be positive and below 2^31");
  if (x->words != W) return fail(PGPU_ERR_INVALID_PARAM, "spmv error: ciphertext width mismatch");
  if (w->mont || w->pair_l2) return fail(PGPU_ERR_INVALID_PARAM, "spmv error: the weights must be a plain uploaded batch");
  if (row_ptr[0] != 0) return fail(PGPU_ERR_INVALID_PARAM, "spmv error: row_ptr[0] must be 0");
  for (size_t i = 0; i < rows; ++i)
    if (row_ptr[i + 1] < row_ptr[i]) return fail(PGPU_ERR_INVALID_PARAM, "spmv error: row_ptr must be non-decreasing");
  if (row_ptr[rows] == 0) return fail(PGPU_ERR_INVALID_PARAM, "spmv error: the matrix has no entries (nnz == 0)");
  if (row_ptr[rows] >= kMax) return fail(PGPU_ERR_INVALID_PARAM, "spmv error: nnz must stay below 2^31");
  const size_t nnz = (size_t)row_ptr[rows];
  if (w->count != nnz) return fail(PGPU_ERR_INVALID_PARAM, "spmv error: Size mismatch! (the weights must hold row_ptr[rows] values)");
  for (size_t t = 0; t < nnz; ++t)
    if (col_idx[t] >= cols) return fail(PGPU_ERR_INVALID_PARAM, "spmv error: a column index is not below count(x)");
  if (e_bits < 1 || e_bits > 64 * w->words) return fail(PGPU_ERR_INVALID_PARAM, "spmv error: e_bits outside the rows of the weight batch");
  if (!same_domain(x->mont, key->nsq)) return fail(PGPU_ERR_INVALID_PARAM, "spmv error: batch belongs to a different key");
  if (rt::pool_size() > 1)
    return fail(PGPU_ERR_UNSUPPORTED, "spmv: pools of more than one GPU are not supported (rows are not sharded yet)");
  const pgpu_pubkey::PubForm* pf = pair_form(key);
  if (!pf || !pgpu::spmv_has(pf->H, pf->K))
    return fail(PGPU_ERR_UNSUPPORTED, "spmv: key has no pair form (1024- to 3072-bit keys; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0 switch it off)");
  // the window tables are addressed by the caller's plaintext column numbers and by digits of the caller's plaintext
  // weights: indexed access.  Under the masked policy the call is refused rather than quietly breaking that promise.
  if (g_ct_gather.load())
    return fail(PGPU_ERR_UNSUPPORTED, "spmv: the masked table-gather policy is on (pgpu_set_table_gather_policy / PGPU_CT_GATHER) and "
                                      "this call indexes its window tables by the plaintext column numbers and by digits of the "
                                      "plaintext weights; no masked variant exists");
  if (x->pair_l2 && (x->pair_l2 != pf->H * pf->K || !(x->pair_form->n == key->n)))
    return fail(PGPU_ERR_INVALID_PARAM, "spmv error: batch belongs to a different key");
  // the plan, on the host: chain descriptors, then the fold levels over the partial rows
  const int G = pf->H, K = pf->K, l2 = G * K;
  const size_t LQ = (size_t)2 * l2, row_bytes = LQ * sizeof(uint32_t);
  policy::SpmvPlan plan;
  if (!policy::spmv_plan(row_ptr, rows, policy::spmv_chunk(G, nnz, rows), &plan))
    return fail(PGPU_ERR_INVALID_PARAM, "spmv error: more chains than a 32-bit descriptor addresses");
  const int win = policy::spmv_window(rows, cols, nnz, plan.n_chains, e_bits, row_bytes);
  // one image for the device: the column indices, then the descriptors of the chains and of every fold level
  const size_t idx_bytes = (nnz * sizeof(uint32_t) + 15) & ~(size_t)15;
  // partial rows: the chains write region 0, fold level f reads region f & 1 and writes the other one
  size_t image_bytes = idx_bytes + plan.chains.size() * sizeof(pgpu::SegsumChunk), region[2] = {plan.partial_rows, 0};
  for (size_t f = 0; f < plan.fold.levels.size(); ++f) {
    image_bytes += plan.fold.levels[f].chunks.size() * sizeof(pgpu::SegsumChunk);
    region[(f + 1) & 1] = std::max(region[(f + 1) & 1], plan.fold.levels[f].partial_rows);
  }
  std::vector<char> image(image_bytes, 0);
  std::memcpy(image.data(), col_idx, nnz * sizeof(uint32_t));
  {
    size_t at = idx_bytes;
    std::memcpy(image.data() + at, plan.chains.data(), plan.chains.size() * sizeof(pgpu::SegsumChunk));
    at += plan.chains.size() * sizeof(pgpu::SegsumChunk);
    for (const auto& lv : plan.fold.levels) {
      std::memcpy(image.data() + at, lv.chunks.data(), lv.chunks.size() * sizeof(pgpu::SegsumChunk));
      at += lv.chunks.size() * sizeof(pgpu::SegsumChunk);
    }
  }
  std::unique_ptr<pgpu_batch> tx;
  RC_TRY(as_pair_batch(key, x, &x, &tx));
  std::unique_ptr<pgpu_batch> o;
  RC_TRY(new_batch(rows, W, &o, l2, x->lane));
  o->pair_form = pair_form_shared(key);
  rt::Device& dev = rt::device(0);
  rt::DeviceGuard g(dev.ordinal);
  hipStream_t s = dev.bs(x->lane);
  RC_TRY(lanes_order(w, x->lane, true));
  // table, plan image and partial rows: the block arena, on the lane's stream like the operands themselves -- what the
  // arena hands out again it hands to this stream, behind the kernels below
  rt::DevMem table, dimage, partial;
  RC_TRY(table.alloc(dev, s, cols * ((size_t)1 << win) * row_bytes));
  RC_TRY(dimage.alloc(dev, s, image_bytes));
  if (region[0]) RC_TRY(partial.alloc(dev, s, (region[0] + region[1]) * row_bytes));
  if (image_bytes <= kBounceBytes) {
    Bounce& bn = bounce();
    RC_TRY(bn.ready());
    std::memcpy(bn.p, image.data(), image_bytes);
    HIP_TRY(hipMemcpyAsync(dimage.p, bn.p, image_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(bn.ev, s));
    bn.pending = true;
  } else {   // through a worker lane's staging buffers, queued on the same stream: nothing is waited for
    rt::TaskGroup tg;
    void* dst = dimage.p;
    const char* src = image.data();
    tg.run(dev, [=](rt::Lane& lane) -> int { return lane.h2d(dst, src, image_bytes, s); });
    RC_TRY(tg.wait());
  }
  const size_t ipw = 64 / (size_t)G;
  auto blocks_of = [](size_t waves) { return (unsigned)((waves + pgpu::kWavesPerWG - 1) / pgpu::kWavesPerWG); };
  {
    // the unchanged table build of the matvec: T[j][d] = x[j]^d for every column of x
    pgpu::MatvecArgs ta{};
    ta.ctx = hensel_pub_view(pf, dev.index);
    ta.x = x->prow(0);
    ta.table = (uint32_t*)table.p;
    ta.window = win;
    ta.cols = cols;
    TimerScope t(dev, s, PGPU_KERNEL_SPMV, PGPU_FORM_SEQ);
    if (!pgpu::launch_matvec_table(G, K, ta, blocks_of((cols + ipw - 1) / ipw), s))
      return fail(PGPU_ERR_UNSUPPORTED, "spmv kernels not compiled for this key class");
    HIP_TRY(hipGetLastError());
    t.stop();
  }
  uint32_t* const reg[2] = {(uint32_t*)partial.p, partial.p ? (uint32_t*)partial.p + region[0] * LQ : nullptr};
  size_t at = idx_bytes;
  {
    pgpu::SpmvArgs a{};
    a.ctx = hensel_pub_view(pf, dev.index);
    a.table = (const uint32_t*)table.p;
    a.col_idx = (const uint32_t*)dimage.p;
    a.w = w->ptr(0);
    a.w_stride = (size_t)w->words;
    a.w_words = w->words;
    a.e_bits = e_bits;
    a.window = win;
    a.chunks = (const pgpu::SegsumChunk*)((const char*)dimage.p + at);
    a.n_chunks = plan.chains.size();
    a.out = o->prow(0);
    a.partial = reg[0];
    TimerScope t(dev, s, PGPU_KERNEL_SPMV, PGPU_FORM_SEQ);
    if (!pgpu::launch_spmv(G, K, a, blocks_of((a.n_chunks + ipw - 1) / ipw), s))
      return fail(PGPU_ERR_UNSUPPORTED, "spmv kernels not compiled for this key class");
    HIP_TRY(hipGetLastError());
    t.stop();
    at += plan.chains.size() * sizeof(pgpu::SegsumChunk);
  }
  // the fold levels: the segmented sum's kernel over the partial rows (perm == null), in the form with the same limbs per
  // half on more lanes where the level leaves SIMDs empty (2048-bit keys: (8,9))
  const pgpu_pubkey::PubForm* wide = nullptr;
  for (const auto& alt : key->hforms)
    if (alt->H * alt->K == l2 && alt->H > G && pgpu::segsum_wide_has(alt->H, alt->K)) wide = alt.get();
  for (size_t f = 0; f < plan.fold.levels.size(); ++f) {
    const auto& lv = plan.fold.levels[f];
    const pgpu_pubkey::PubForm* lf = wide && policy::segsum_wide_pays(wide->H, lv.chunks.size()) ? wide : pf;
    pgpu::SegsumArgs a{};
    a.ctx = hensel_pub_view(lf, dev.index);
    a.src = reg[f & 1];
    a.perm = nullptr;
    a.chunks = (const pgpu::SegsumChunk*)((const char*)dimage.p + at);
    a.n_chunks = lv.chunks.size();
    a.out = o->prow(0);
    a.partial = reg[(f + 1) & 1];
    const size_t fipw = 64 / (size_t)lf->H, waves = (a.n_chunks + fipw - 1) / fipw;
    TimerScope t(dev, s, PGPU_KERNEL_SPMV, PGPU_FORM_SEQ);
    if (!pgpu::launch_segsum(lf->H, lf->K, a, blocks_of(waves), s))
      return fail(PGPU_ERR_UNSUPPORTED, "segment sum kernels not compiled for this key class");
    HIP_TRY(hipGetLastError());
    t.stop();
    at += lv.chunks.size() * sizeof(pgpu::SegsumChunk);
  }
  RC_TRY(lanes_order(w, x->lane, false));
  *out = o.release();
  return PGPU_OK;
}

// ---- encrypted weighted sum of K resident batches (hensel_wsum.hpp; policy.hpp: wsum_*) ----
int pgpu_ct_weighted_sum_plan(int key_bits, size_t count, size_t n_terms, const uint64_t* weights_or_null, int w_words,
                              int* lanes, int* limbs, int* slices, size_t* steps, size_t* products) {
  if (key_bits < 1 || count == 0 || n_terms == 0 || n_terms > policy::kWsumMaxTerms || (weights_or_null && w_words < 1))
    return fail(PGPU_ERR_INVALID_PARAM, "weighted sum plan: key_bits, count and n_terms must be positive, n_terms at most 65535, "
                                        "w_words positive where weights are given");
  int G = 0, K = 0;
  if (!policy::matvec_geometry(key_bits, &G, &K))
    return fail(PGPU_ERR_UNSUPPORTED, "weighted sum: keys of this size have no pair rows (1024- to 3072-bit key classes only)");
  policy::WsumPlan plan;
  if (!policy::wsum_plan(weights_or_null, w_words, n_terms, policy::wsum_slices(G, count, n_terms, !weights_or_null), &plan))
    return fail(PGPU_ERR_INVALID_PARAM, "weighted sum plan: a schedule of 2^31 steps or more");
  if (plan.products && count > ~(size_t)0 / plan.products)
    return fail(PGPU_ERR_INVALID_PARAM, "weighted sum plan: the product count overflows");
  policy::wsum_geometry(key_bits, count * plan.slices.size(), &G, &K);
  if (lanes) *lanes = G;
  if (limbs) *limbs = K;
  if (slices) *slices = (int)plan.slices.size();
  if (steps) *steps = plan.longest;
  if (products) *products = count * plan.products;
  return PGPU_OK;
}

int pgpu_batch_ct_weighted_sum(const pgpu_pubkey* key, const pgpu_batch* const* xs, size_t n_terms, const uint64_t* weights,
                               int w_words, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !xs || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  if (n_terms == 0 || n_terms > policy::kWsumMaxTerms)
    return fail(PGPU_ERR_INVALID_PARAM, "weighted sum error: n_terms must be between 1 and 65535");
  if (weights && w_words < 1) return fail(PGPU_ERR_INVALID_PARAM, "weighted sum error: w_words must be positive");
  const int W = 2 * key->n_words;
  for (size_t k = 0; k < n_terms; ++k) {
    if (!xs[k]) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
    RC_TRY(check_gen(xs[k]->gen, "batch"));
  }
  const size_t count = xs[0]->count;
  if (count == 0) return fail(PGPU_ERR_INVALID_PARAM, "weighted sum error: empty batch");
  for (size_t k = 0; k < n_terms; ++k) {
    if (xs[k]->count != count) return fail(PGPU_ERR_INVALID_PARAM, "weighted sum error: Size mismatch! (every batch must hold count(xs[0]) elements)");
    if (xs[k]->words != W) return fail(PGPU_ERR_INVALID_PARAM, "weighted sum error: ciphertext width mismatch");
    if (!same_domain(xs[k]->mont, key->nsq)) return fail(PGPU_ERR_INVALID_PARAM, "weighted sum error: batch belongs to a different key");
  }
  if (rt::pool_size() > 1)
    return fail(PGPU_ERR_UNSUPPORTED, "weighted sum: pools of more than one GPU are not supported (elements are not sharded yet)");
  const pgpu_pubkey::PubForm* pf = pair_form(key);
  if (!pf || !pgpu::matvec_has(pf->H, pf->K))
    return fail(PGPU_ERR_UNSUPPORTED, "weighted sum: key has no pair form (1024- to 3072-bit keys; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0 switch it off)");
  // the schedule and the row addresses depend on the caller's PLAINTEXT weights only (never on key material or on anything
  // encrypted); the call is refused under the masked policy all the same, like its siblings: one rule for the aggregation calls
  if (g_ct_gather.load())
    return fail(PGPU_ERR_UNSUPPORTED, "weighted sum: the masked table-gather policy is on (pgpu_set_table_gather_policy / PGPU_CT_GATHER); "
                                      "the schedule and the row addresses depend on the caller's plaintext weights only, but "
                                      "the aggregation calls on resident ciphertexts have no masked variant");
  for (size_t k = 0; k < n_terms; ++k)
    if (xs[k]->pair_l2 && (xs[k]->pair_l2 != pf->H * pf->K || !(xs[k]->pair_form->n == key->n)))
      return fail(PGPU_ERR_INVALID_PARAM, "weighted sum error: batch belongs to a different key");
  // the schedule, on the host: the slices of the terms, then the fold over their partial rows
  const int G = pf->H, l2 = G * pf->K;
  const size_t LQ = (size_t)2 * l2, row_bytes = LQ * sizeof(uint32_t);
  policy::WsumPlan plan, fold;
  if (!policy::wsum_plan(weights, w_words, n_terms, policy::wsum_slices(G, count, n_terms, !weights), &plan))
    return fail(PGPU_ERR_INVALID_PARAM, "weighted sum error: a schedule of 2^31 steps or more");
  const size_t S = plan.slices.size();
  if (S > 1) policy::wsum_plan(nullptr, 0, S, 1, &fold);
  // the operands as pair rows, every used batch converted once on its own lane; a batch of weight zero is never read
  std::vector<char> used(n_terms, 0);
  if (!plan.all_zero)
    for (const pgpu::WsumSlice& sl : plan.slices) {
      used[sl.first] = 1;
      for (size_t t = 0; t < sl.n_steps; ++t) {
        const pgpu::WsumStep& st = plan.steps[(size_t)sl.step_begin + t];
        if (st.op != pgpu::kWsumSqr) used[st.op] = 1;
      }
    }
  std::vector<std::unique_ptr<pgpu_batch>> tmps;
  std::map<const pgpu_batch*, const pgpu_batch*> pair_of;    // (the same handle may appear more than once)
  for (size_t k = 0; k < n_terms; ++k) {
    if (!used[k] || pair_of.count(xs[k])) continue;
    const pgpu_batch* p = nullptr;
    std::unique_ptr<pgpu_batch> t;
    RC_TRY(as_pair_batch(key, xs[k], &p, &t));
    if (t) tmps.push_back(std::move(t));
    pair_of[xs[k]] = p;
  }
  const int lane = xs[0]->lane;
  std::unique_ptr<pgpu_batch> o;
  RC_TRY(new_batch(count, W, &o, l2, lane));
  o->pair_form = pair_form_shared(key);
  rt::Device& dev = rt::device(0);
  rt::DeviceGuard g(dev.ordinal);
  hipStream_t s = dev.bs(lane);
  for (const auto& kv : pair_of) RC_TRY(lanes_order(kv.second, lane, true));
  // one image for the device: the row bases, the slice descriptors of both launches, their step lists
  rt::DevMem dimage, partial;
  if (S > 1) RC_TRY(partial.alloc(dev, s, (S - 1) * count * row_bytes));
  const size_t tab_bytes = n_terms * sizeof(uint32_t*), ftab_bytes = (S > 1 ? S : 0) * sizeof(uint32_t*);
  const size_t sl_at = tab_bytes + ftab_bytes, fsl_at = sl_at + S * sizeof(pgpu::WsumSlice);
  const size_t st_at = fsl_at + fold.slices.size() * sizeof(pgpu::WsumSlice);
  const size_t fst_at = st_at + plan.steps.size() * sizeof(pgpu::WsumStep);
  const size_t image_bytes = fst_at + fold.steps.size() * sizeof(pgpu::WsumStep);
  std::vector<char> image(image_bytes, 0);
  {
    // every entry of the table is addressable: a batch that no step names stands in as the result batch itself
    std::vector<const uint32_t*> tab(n_terms, o->prow(0)), ftab;
    for (size_t k = 0; k < n_terms; ++k)
      if (used[k]) tab[k] = pair_of[xs[k]]->prow(0);
    std::memcpy(image.data(), tab.data(), tab_bytes);
    // slice 0 writes the result batch, the others a partial region each; the fold multiplies them into the result batch in
    // place (a group reads row i of every region before it stores row i, and no other live group touches that row)
    for (size_t j = 0; j < S; ++j) {
      plan.slices[j].dst = j == 0 ? o->prow(0) : (uint32_t*)partial.p + (j - 1) * count * LQ;
      ftab.push_back(plan.slices[j].dst);
    }
    if (S > 1) {
      std::memcpy(image.data() + tab_bytes, ftab.data(), ftab_bytes);
      fold.slices[0].dst = o->prow(0);
      std::memcpy(image.data() + fsl_at, fold.slices.data(), sizeof(pgpu::WsumSlice));
      std::memcpy(image.data() + fst_at, fold.steps.data(), fold.steps.size() * sizeof(pgpu::WsumStep));
    }
    std::memcpy(image.data() + sl_at, plan.slices.data(), S * sizeof(pgpu::WsumSlice));
    if (!plan.steps.empty()) std::memcpy(image.data() + st_at, plan.steps.data(), plan.steps.size() * sizeof(pgpu::WsumStep));
  }
  RC_TRY(dimage.alloc(dev, s, image_bytes));
  if (image_bytes <= kBounceBytes) {
    Bounce& bn = bounce();
    RC_TRY(bn.ready());
    std::memcpy(bn.p, image.data(), image_bytes);
    HIP_TRY(hipMemcpyAsync(dimage.p, bn.p, image_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(bn.ev, s));
    bn.pending = true;
  } else {   // through a worker lane's staging buffers, queued on the same stream: nothing is waited for
    rt::TaskGroup tg;
    void* dst = dimage.p;
    const char* src = image.data();
    tg.run(dev, [=](rt::Lane& ln) -> int { return ln.h2d(dst, src, image_bytes, s); });
    RC_TRY(tg.wait());
  }
  // the form with the same limbs per half on more lanes, for launches that leave SIMDs empty (policy.hpp: wsum_wide_pays)
  const pgpu_pubkey::PubForm* wide = nullptr;
  for (const auto& alt : key->hforms)
    if (alt->H * alt->K == l2 && alt->H > G && pgpu::wsum_wide_has(alt->H, alt->K)) wide = alt.get();
  auto launch = [&](size_t tab_off, size_t slices_off, size_t steps_off, size_t n_slices) -> int {
    const pgpu_pubkey::PubForm* lf = wide && policy::wsum_wide_pays(wide->H, count * n_slices) ? wide : pf;
    pgpu::WsumArgs a{};
    a.ctx = hensel_pub_view(lf, dev.index);
    a.rows = (const uint32_t* const*)((const char*)dimage.p + tab_off);
    a.slices = (const pgpu::WsumSlice*)((const char*)dimage.p + slices_off);
    a.steps = (const pgpu::WsumStep*)((const char*)dimage.p + steps_off);
    a.count = count;
    const size_t ipw = 64 / (size_t)lf->H, waves = (count + ipw - 1) / ipw;
    TimerScope t(dev, s, PGPU_KERNEL_WSUM, PGPU_FORM_SEQ);
    if (!pgpu::launch_wsum(lf->H, lf->K, a, (unsigned)((waves + pgpu::kWavesPerWG - 1) / pgpu::kWavesPerWG), (unsigned)n_slices, s))
      return fail(PGPU_ERR_UNSUPPORTED, "weighted sum kernels not compiled for this key class");
    HIP_TRY(hipGetLastError());
    t.stop();
    return PGPU_OK;
  };
  RC_TRY(launch(0, sl_at, st_at, S));
  if (S > 1) RC_TRY(launch(tab_bytes, fsl_at, fst_at, 1));
  for (const auto& kv : pair_of) RC_TRY(lanes_order(kv.second, lane, false));
  *out = o.release();
  return PGPU_OK;
}

// ---- encrypted segmented prefix sum (hensel_segscan.hpp; policy.hpp: segscan_*) ----
int pgpu_ct_segment_scan_plan(int key_bits, size_t rows, size_t seg_len, int* chunk, int* levels, size_t* products) {
  if (key_bits < 1 || rows == 0 || seg_len == 0)
    return fail(PGPU_ERR_INVALID_PARAM, "segment scan plan: key_bits, rows and seg_len must be positive");
  int G = 0, K = 0;
  if (!policy::matvec_geometry(key_bits, &G, &K))
    return fail(PGPU_ERR_UNSUPPORTED, "segment scan: keys of this size have no pair rows (1024- to 3072-bit key classes only)");
  const int c = policy::segscan_chunk(G, rows, seg_len);
  if (!policy::segscan_fits(c, rows, seg_len))
    return fail(PGPU_ERR_INVALID_PARAM, "segment scan plan: more chunks than a 32-bit carry index addresses");
  if (chunk) *chunk = c;
  if (levels) *levels = policy::segscan_levels(c, seg_len);
  if (products) *products = policy::segscan_products(c, rows, seg_len);
  return PGPU_OK;
}

int pgpu_batch_ct_segment_scan(const pgpu_pubkey* key, const pgpu_batch* x, size_t seg_len, unsigned flags, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !x || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(x->gen, "batch"));
  const int W = 2 * key->n_words;
  const size_t count = x->count;
  if (seg_len == 0 || count == 0 || count % seg_len != 0)
    return fail(PGPU_ERR_INVALID_PARAM, "segment scan error: seg_len must be positive and divide count(x)");
  if (flags & ~PGPU_SCAN_REVERSE) return fail(PGPU_ERR_INVALID_PARAM, "segment scan error: unknown flag bit (PGPU_SCAN_REVERSE is the only one)");
  if (x->words != W) return fail(PGPU_ERR_INVALID_PARAM, "segment scan error: ciphertext width mismatch");
  if (!same_domain(x->mont, key->nsq)) return fail(PGPU_ERR_INVALID_PARAM, "segment scan error: batch belongs to a different key");
  if (rt::pool_size() > 1)
    return fail(PGPU_ERR_UNSUPPORTED, "segment scan: pools of more than one GPU are not supported (rows are not sharded yet)");
  const pgpu_pubkey::PubForm* pf = pair_form(key);
  if (!pf || !pgpu::matvec_has(pf->H, pf->K))
    return fail(PGPU_ERR_UNSUPPORTED, "segment scan: key has no pair form (1024- to 3072-bit keys; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0 switch it off)");
  // the address stream here depends on rows, seg_len and the plan alone; the call is refused under the masked policy all
  // the same, like its two siblings: one rule for the aggregation calls
  if (g_ct_gather.load())
    return fail(PGPU_ERR_UNSUPPORTED, "segment scan: the masked table-gather policy is on (pgpu_set_table_gather_policy / PGPU_CT_GATHER); "
                                      "the aggregation calls on resident ciphertexts have no masked variant");
  if (x->pair_l2 && (x->pair_l2 != pf->H * pf->K || !(x->pair_form->n == key->n)))
    return fail(PGPU_ERR_INVALID_PARAM, "segment scan error: batch belongs to a different key");
  // the plan, on the host
  const int G = pf->H, K = pf->K, l2 = G * K;
  const size_t LQ = (size_t)2 * l2, row_bytes = LQ * sizeof(uint32_t), rows = count / seg_len;
  const int chunk = policy::segscan_chunk(G, rows, seg_len);
  if (!policy::segscan_fits(chunk, rows, seg_len))
    return fail(PGPU_ERR_INVALID_PARAM, "segment scan error: more chunks than a 32-bit carry index addresses (a larger PGPU_SEGSCAN_CHUNK, or fewer rows per call)");
  policy::SegscanPlan plan;
  policy::segscan_plan(rows, seg_len, chunk, (flags & PGPU_SCAN_REVERSE) != 0, &plan);
  static_assert(sizeof(pgpu::SegsumChunk) == 16 && sizeof(pgpu::SegscanChunk) == 16, "descriptors are packed into one image");
  // one image for the device: per level the up-sweep descriptors, then the scan descriptors.  Scratch rows: per level but
  // the deepest its totals and, beside them, the carries the level below makes of them
  const size_t nl = plan.levels.size();
  size_t image_bytes = 0, scratch_rows = 0;
  std::vector<size_t> up_at(nl), scan_at(nl), totals_at(nl), carry_at(nl);
  for (size_t l = 0; l < nl; ++l) {
    const auto& lv = plan.levels[l];
    up_at[l] = image_bytes;
    image_bytes += lv.up.size() * sizeof(pgpu::SegsumChunk);
    scan_at[l] = image_bytes;
    image_bytes += lv.scan.size() * sizeof(pgpu::SegscanChunk);
    totals_at[l] = scratch_rows;
    carry_at[l] = scratch_rows + lv.totals;
    scratch_rows += 2 * lv.totals;
  }
  std::vector<char> image(image_bytes, 0);
  for (size_t l = 0; l < nl; ++l) {
    const auto& lv = plan.levels[l];
    if (!lv.up.empty()) std::memcpy(image.data() + up_at[l], lv.up.data(), lv.up.size() * sizeof(pgpu::SegsumChunk));
    std::memcpy(image.data() + scan_at[l], lv.scan.data(), lv.scan.size() * sizeof(pgpu::SegscanChunk));
  }
  std::unique_ptr<pgpu_batch> tx;
  RC_TRY(as_pair_batch(key, x, &x, &tx));
  std::unique_ptr<pgpu_batch> o;
  RC_TRY(new_batch(count, W, &o, l2, x->lane));
  o->pair_form = pair_form_shared(key);
  rt::Device& dev = rt::device(0);
  rt::DeviceGuard g(dev.ordinal);
  hipStream_t s = dev.bs(x->lane);
  // plan image, totals and carries: the block arena, on the lane's stream like the operands themselves -- what the arena
  // hands out again it hands to this stream, behind the kernels below
  rt::DevMem dimage, scratch;
  RC_TRY(dimage.alloc(dev, s, image_bytes));
  if (scratch_rows) RC_TRY(scratch.alloc(dev, s, scratch_rows * row_bytes));
  if (image_bytes <= kBounceBytes) {
    Bounce& bn = bounce();
    RC_TRY(bn.ready());
    std::memcpy(bn.p, image.data(), image_bytes);
    HIP_TRY(hipMemcpyAsync(dimage.p, bn.p, image_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(bn.ev, s));
    bn.pending = true;
  } else {   // through a worker lane's staging buffers, queued on the same stream: nothing is waited for
    rt::TaskGroup tg;
    void* dst = dimage.p;
    const char* src = image.data();
    tg.run(dev, [=](rt::Lane& lane) -> int { return lane.h2d(dst, src, image_bytes, s); });
    RC_TRY(tg.wait());
  }
  // the form with the same limbs per half on more lanes, for the up-sweeps that leave SIMDs empty (segsum_kernel only)
  const pgpu_pubkey::PubForm* wide = nullptr;
  for (const auto& alt : key->hforms)
    if (alt->H * alt->K == l2 && alt->H > G && pgpu::segsum_wide_has(alt->H, alt->K)) wide = alt.get();
  uint32_t* const sc = (uint32_t*)scratch.p;
  // level l reads in(l) and writes res(l): x and the result batch, or the totals and the carries of the level above
  auto in = [&](size_t l) -> const uint32_t* { return l == 0 ? x->prow(0) : sc + totals_at[l - 1] * LQ; };
  auto res = [&](size_t l) -> uint32_t* { return l == 0 ? o->prow(0) : sc + carry_at[l - 1] * LQ; };
  for (size_t l = 0; l + 1 < nl; ++l) {   // up-sweep: the chunk totals, level by level
    const auto& lv = plan.levels[l];
    const pgpu_pubkey::PubForm* lf = wide && policy::segsum_wide_pays(wide->H, lv.up.size()) ? wide : pf;
    pgpu::SegsumArgs a{};
    a.ctx = hensel_pub_view(lf, dev.index);
    a.src = in(l);
    a.perm = nullptr;
    a.chunks = (const pgpu::SegsumChunk*)((const char*)dimage.p + up_at[l]);
    a.n_chunks = lv.up.size();
    a.out = nullptr;                       // (every descriptor names a row of partial)
    a.partial = sc + totals_at[l] * LQ;
    const size_t ipw = 64 / (size_t)lf->H, waves = (a.n_chunks + ipw - 1) / ipw;
    TimerScope t(dev, s, PGPU_KERNEL_SEGSCAN, PGPU_FORM_SEQ);
    if (!pgpu::launch_segsum(lf->H, lf->K, a, (unsigned)((waves + pgpu::kWavesPerWG - 1) / pgpu::kWavesPerWG), s))
      return fail(PGPU_ERR_UNSUPPORTED, "segment sum kernels not compiled for this key class");
    HIP_TRY(hipGetLastError());
    t.stop();
  }
  for (size_t l = nl; l-- > 0;) {         // down-sweep: the deepest level has no carries, every other one those below it
    const auto& lv = plan.levels[l];
    pgpu::SegscanArgs a{};
    a.ctx = hensel_pub_view(pf, dev.index);
    a.src = in(l);
    a.carry = l + 1 < nl ? res(l + 1) : nullptr;
    a.chunks = (const pgpu::SegscanChunk*)((const char*)dimage.p + scan_at[l]);
    a.n_chunks = lv.scan.size();
    a.out = res(l);
    a.step = lv.reverse ? -1 : 1;
    const size_t ipw = 64 / (size_t)G, waves = (a.n_chunks + ipw - 1) / ipw;
    TimerScope t(dev, s, PGPU_KERNEL_SEGSCAN, PGPU_FORM_SEQ);
    if (!pgpu::launch_segscan(G, K, a, (unsigned)((waves + pgpu::kWavesPerWG - 1) / pgpu::kWavesPerWG), s))
      return fail(PGPU_ERR_UNSUPPORTED, "segment scan kernels not compiled for this key class");
    HIP_TRY(hipGetLastError());
    t.stop();
  }
  *out = o.release();
  return PGPU_OK;
}

// ---- encrypted slot packing (hensel_pack.hpp) ----
// seg_len * slot_bits <= cap, without forming the product
static bool pack_fits(size_t seg_len, int slot_bits, int cap) {
  return seg_len >= 1 && slot_bits >= 1 && cap >= 1 && slot_bits <= cap && seg_len <= (size_t)(cap / slot_bits);
}

int pgpu_ct_pack_plan(int key_bits, size_t rows, size_t seg_len, int slot_bits, int* lanes, int* limbs, size_t* products) {
  if (key_bits < 1 || rows == 0 || seg_len == 0 || slot_bits < 1)
    return fail(PGPU_ERR_INVALID_PARAM, "pack plan: key_bits, rows, seg_len and slot_bits must be positive");
  if (!pack_fits(seg_len, slot_bits, key_bits - 1))
    return fail(PGPU_ERR_INVALID_PARAM, "pack plan: seg_len * slot_bits exceeds key_bits - 1 (the packed plaintext would wrap modulo n)");
  int G = 0, K = 0;
  if (!policy::pack_geometry(key_bits, rows, &G, &K))
    return fail(PGPU_ERR_UNSUPPORTED, "pack: keys of this size have no pair rows (1024- to 3072-bit key classes only)");
  const size_t per_row = (seg_len - 1) * ((size_t)slot_bits + 1);   // (both factors are below key_bits)
  if (per_row && rows > ~(size_t)0 / per_row) return fail(PGPU_ERR_INVALID_PARAM, "pack plan: the product count overflows");
  if (lanes) *lanes = G;
  if (limbs) *limbs = K;
  if (products) *products = rows * per_row;
  return PGPU_OK;
}

int pgpu_batch_ct_pack(const pgpu_pubkey* key, const pgpu_batch* x, size_t seg_len, int slot_bits, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !x || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(x->gen, "batch"));
  const int W = 2 * key->n_words;
  const size_t count = x->count;
  if (seg_len == 0 || count == 0 || count % seg_len != 0)
    return fail(PGPU_ERR_INVALID_PARAM, "pack error: seg_len must be positive and divide count(x)");
  if (slot_bits < 1) return fail(PGPU_ERR_INVALID_PARAM, "pack error: slot_bits must be positive");
  if (!pack_fits(seg_len, slot_bits, key->n.BitSize() - 1))
    return fail(PGPU_ERR_INVALID_PARAM, "pack error: seg_len * slot_bits exceeds bitlen(n) - 1 (the packed plaintext would wrap modulo n)");
  if (x->words != W) return fail(PGPU_ERR_INVALID_PARAM, "pack error: ciphertext width mismatch");
  if (!same_domain(x->mont, key->nsq)) return fail(PGPU_ERR_INVALID_PARAM, "pack error: batch belongs to a different key");
  if (rt::pool_size() > 1)
    return fail(PGPU_ERR_UNSUPPORTED, "pack: pools of more than one GPU are not supported (rows are not sharded yet)");
  const pgpu_pubkey::PubForm* pf = pair_form(key);
  if (!pf || !pgpu::matvec_has(pf->H, pf->K))
    return fail(PGPU_ERR_UNSUPPORTED, "pack: key has no pair form (1024- to 3072-bit keys; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0 switch it off)");
  // the address stream here depends on rows and seg_len alone; the call is refused under the masked policy all the same,
  // like its three siblings: one rule for the aggregation calls
  if (g_ct_gather.load())
    return fail(PGPU_ERR_UNSUPPORTED, "pack: the masked table-gather policy is on (pgpu_set_table_gather_policy / PGPU_CT_GATHER); "
                                      "the aggregation calls on resident ciphertexts have no masked variant");
  if (x->pair_l2 && (x->pair_l2 != pf->H * pf->K || !(x->pair_form->n == key->n)))
    return fail(PGPU_ERR_INVALID_PARAM, "pack error: batch belongs to a different key");
  const int G = pf->H, l2 = G * pf->K;
  const size_t rows = count / seg_len;
  std::unique_ptr<pgpu_batch> tx;
  RC_TRY(as_pair_batch(key, x, &x, &tx));
  std::unique_ptr<pgpu_batch> o;
  RC_TRY(new_batch(rows, W, &o, l2, x->lane));
  o->pair_form = pair_form_shared(key);
  rt::Device& dev = rt::device(0);
  rt::DeviceGuard g(dev.ordinal);
  hipStream_t s = dev.bs(x->lane);
  // the form with the same limbs per half on more lanes, for launches that leave SIMDs empty (policy.hpp: pack_wide_pays)
  const pgpu_pubkey::PubForm* lf = pf;
  for (const auto& alt : key->hforms)
    if (alt->H * alt->K == l2 && alt->H > G && pgpu::pack_wide_has(alt->H, alt->K) && policy::pack_wide_pays(alt->H, rows)) lf = alt.get();
  pgpu::PackArgs a{};
  a.ctx = hensel_pub_view(lf, dev.index);
  a.src = x->prow(0);
  a.rows = rows;
  a.seg_len = (uint32_t)seg_len;     // (both at most bitlen(n) - 1)
  a.slot_bits = (uint32_t)slot_bits;
  a.out = o->prow(0);
  const size_t ipw = 64 / (size_t)lf->H, waves = (rows + ipw - 1) / ipw;
  TimerScope t(dev, s, PGPU_KERNEL_PACK, PGPU_FORM_SEQ);
  if (!pgpu::launch_pack(lf->H, lf->K, a, (unsigned)((waves + pgpu::kWavesPerWG - 1) / pgpu::kWavesPerWG), s))
    return fail(PGPU_ERR_UNSUPPORTED, "pack kernels not compiled for this key class");
  HIP_TRY(hipGetLastError());
  t.stop();
  *out = o.release();
  return PGPU_OK;
}

int pgpu_set_batch_lane(int lane) {
  if (lane < 0 || lane >= rt::kBatchLanes) return fail(PGPU_ERR_INVALID_PARAM, "batch lane out of range (pgpu_batch_lanes())");
  t_batch_lane = lane;
  t_lane_explicit = true;
  return PGPU_OK;
}
int pgpu_batch_lane(const pgpu_batch* b) { return b ? b->lane : 0; }
int pgpu_batch_is_current(const pgpu_batch* b) { return b && rt::pool_size() > 0 && b->gen == rt::pool_generation() ? 1 : 0; }
int pgpu_batch_lanes(void) { return rt::kBatchLanes; }
int pgpu_batch_row_limbs(const pgpu_batch* b) { return b ? 2 * b->pair_l2 : 0; }
