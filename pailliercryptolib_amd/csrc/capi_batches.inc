// pailliercryptolib_amd -- sharded device-resident batches (pgpu_batch_*): upload / download, encrypt / decrypt, the
// element-wise resident operations, batch lanes.  The aggregation calls (matvec, spmv, weighted sum, segment sum, segment
// scan, pack) are in capi_aggregate.inc.
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
