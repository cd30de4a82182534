// pailliercryptolib_amd -- the aggregation calls on resident ciphertexts (pgpu_batch_ct_matvec / _matvec_bucket / _matmul / _conv2d / _spmv / _weighted_sum /
// _segment_sum / _segment_scan / _pack / _negate / _sub / _matvec_signed / _matmul_signed / _conv2d_signed / _spmv_signed) and their plan queries (pgpu_ct_*_plan).
// Part of the translation unit of capi.cpp (included there, in place, after capi_batches.inc, whose bounce buffer the plan
// upload shares).  Every call is: its own parameter checks, the admission tail, its plan (policy.hpp), the result set-up,
// one upload of the plan image, its launches.  What the calls have in common is written once, in the helpers below.

namespace {
// ---- admission tail: the refusals every aggregation call ends its checks with ----
struct AggOp {
  const char* name;            // the message prefix: "segment sum"
  const char* sharded;         // what a pool would have to shard: "(... are not sharded yet)"
  const char* masked;          // why the masked table-gather policy refuses the call: what follows "... PGPU_CT_GATHER)"
  bool (*has)(int, int);       // the call's kernels are compiled for the pair form
  const char* pair_rows_msg;   // pair rows of another key: null -- "<name> error: batch belongs to a different key"
};
constexpr const char* kNoMaskedVariant = "; the aggregation calls on resident ciphertexts have no masked variant";

int agg_admit(const AggOp& op, const pgpu_pubkey* key, const pgpu_batch* const* xs, size_t n, const pgpu_pubkey::PubForm** form) {
  const auto other_key = [&] { return std::string(op.name) + " error: batch belongs to a different key"; };
  for (size_t k = 0; k < n; ++k)
    if (!same_domain(xs[k]->mont, key->nsq)) return fail(PGPU_ERR_INVALID_PARAM, other_key());
  if (rt::pool_size() > 1)
    return fail(PGPU_ERR_UNSUPPORTED, std::string(op.name) + ": pools of more than one GPU are not supported (" + op.sharded + " are not sharded yet)");
  const pgpu_pubkey::PubForm* pf = pair_form(key);
  if (!pf || !op.has(pf->H, pf->K))
    return fail(PGPU_ERR_UNSUPPORTED, std::string(op.name) + ": key has no pair form (1024- to 3072-bit keys; PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0 switch it off)");
  // every one of these calls addresses rows or window tables by the caller's plaintext (ids, column numbers, digits of
  // weights) or by the plan alone: indexed access.  Under the masked policy the call is refused rather than quietly
  // breaking that promise -- one rule for the aggregation calls, also for those whose addresses depend on sizes only.
  if (g_ct_gather.load())
    return fail(PGPU_ERR_UNSUPPORTED, std::string(op.name) + ": the masked table-gather policy is on (pgpu_set_table_gather_policy / PGPU_CT_GATHER)" + op.masked);
  for (size_t k = 0; k < n; ++k)
    if (xs[k]->pair_l2 && (xs[k]->pair_l2 != pf->H * pf->K || !(xs[k]->pair_form->n == key->n)))
      return fail(PGPU_ERR_INVALID_PARAM, op.pair_rows_msg ? std::string(op.pair_rows_msg) : other_key());
  *form = pf;
  return PGPU_OK;
}

// ---- result set-up: the output batch in pair rows on device 0, its guard and the lane's stream ----
struct AggRun {
  const pgpu_pubkey::PubForm* pf = nullptr;
  std::unique_ptr<pgpu_batch> tx, o;
  const pgpu_batch* x = nullptr;        // the operand as a pair batch (tx holds a converted copy)
  rt::Device* dev = nullptr;
  std::optional<rt::DeviceGuard> guard;
  hipStream_t s = nullptr;
  int open_out(const pgpu_pubkey* key, const pgpu_pubkey::PubForm* form, size_t rows, int lane) {
    pf = form;
    RC_TRY(new_batch(rows, 2 * key->n_words, &o, pf->H * pf->K, lane));
    o->pair_form = pair_form_shared(key);
    dev = &rt::device(0);
    guard.emplace(dev->ordinal);
    s = dev->bs(lane);
    return PGPU_OK;
  }
  int open(const pgpu_pubkey* key, const pgpu_pubkey::PubForm* form, const pgpu_batch* operand, size_t rows) {
    RC_TRY(as_pair_batch(key, operand, &x, &tx));
    return open_out(key, form, rows, x->lane);
  }
  int finish(pgpu_batch** out) {
    *out = o.release();
    return PGPU_OK;
  }
};

// ---- plan image: device memory from the block arena on the lane's stream (what the arena hands out again it hands to this
// stream, behind the kernels), filled through the calling thread's bounce buffer or, beyond it, through a worker lane's
// staging buffers queued on the same stream: nothing is waited for ----
int upload_plan_image(rt::Device& dev, hipStream_t s, const char* bytes, size_t size, rt::DevMem* dimage) {
  RC_TRY(dimage->alloc(dev, s, size));
  if (size <= kBounceBytes) {
    Bounce& bn = bounce();
    RC_TRY(bn.ready());
    std::memcpy(bn.p, bytes, size);
    HIP_TRY(hipMemcpyAsync(dimage->p, bn.p, size, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(bn.ev, s));
    bn.pending = true;
    return PGPU_OK;
  }
  rt::TaskGroup tg;
  void* dst = dimage->p;
  tg.run(dev, [=](rt::Lane& lane) -> int { return lane.h2d(dst, bytes, size, s); });
  return tg.wait();
}

// the form with the same limbs per half on more lanes, for launches that leave SIMDs empty (2048-bit keys: (8,9) beside
// (4,18)); null: the key has none that `has` is compiled for
const pgpu_pubkey::PubForm* wide_form(const pgpu_pubkey* key, const pgpu_pubkey::PubForm* pf, bool (*has)(int, int)) {
  const pgpu_pubkey::PubForm* wide = nullptr;
  for (const auto& alt : key->hforms)
    if (alt->H * alt->K == pf->H * pf->K && alt->H > pf->H && has(alt->H, alt->K)) wide = alt.get();
  return wide;
}

// ---- one timed launch: `sets` x ceil(items / (64 / lanes)) wavefronts in workgroups of kWavesPerWG; launch(blocks) is the
// launch_* trampoline, false where the kernel is not compiled ----
extern "C++" template <class Launch>   // (this part of capi.cpp is inside its extern "C" block)
int timed_launch(const AggRun& r, size_t items, int lanes, int kind, const char* op, Launch&& launch, size_t sets = 1) {
  const size_t ipw = 64 / (size_t)lanes, waves = sets * ((items + ipw - 1) / ipw);
  TimerScope t(*r.dev, r.s, kind, PGPU_FORM_SEQ);
  if (!launch((unsigned)((waves + pgpu::kWavesPerWG - 1) / pgpu::kWavesPerWG)))
    return fail(PGPU_ERR_UNSUPPORTED, std::string(op) + " kernels not compiled for this key class");
  HIP_TRY(hipGetLastError());
  t.stop();
  return PGPU_OK;
}

// ---- one level of segsum_kernel over n chunk descriptors: the segment sum's levels, the spmv's fold levels, the segment
// scan's up-sweeps.  A level whose chains leave SIMDs empty runs in the wide form (policy.hpp: segsum_wide_pays) ----
int segsum_level(const AggRun& r, const pgpu_pubkey::PubForm* wide, const uint32_t* src, const uint32_t* perm, const void* chunks,
                 size_t n, uint32_t* out, uint32_t* partial, int kind) {
  const pgpu_pubkey::PubForm* lf = wide && policy::segsum_wide_pays(wide->H, n) ? wide : r.pf;
  pgpu::SegsumArgs a{};
  a.ctx = hensel_pub_view(lf, r.dev->index);
  a.src = src;
  a.perm = perm;
  a.chunks = (const pgpu::SegsumChunk*)chunks;
  a.n_chunks = n;
  a.out = out;
  a.partial = partial;
  return timed_launch(r, n, lf->H, kind, "segment sum", [&](unsigned blocks) { return pgpu::launch_segsum(lf->H, lf->K, a, blocks, r.s); });
}
}  // namespace

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
  const size_t cols = x->count;
  if (rows == 0) return fail(PGPU_ERR_INVALID_PARAM, "matvec error: rows must be positive");
  if (x->words != 2 * key->n_words) return fail(PGPU_ERR_INVALID_PARAM, "matvec error: ciphertext width mismatch");
  if (w->mont || w->pair_l2) return fail(PGPU_ERR_INVALID_PARAM, "matvec error: the matrix must be a plain uploaded batch");
  if (rows > ~(size_t)0 / cols || w->count != rows * cols)
    return fail(PGPU_ERR_INVALID_PARAM, "matvec error: Size mismatch! (the matrix must hold rows * count(x) values)");
  if (e_bits < 1 || e_bits > 64 * w->words) return fail(PGPU_ERR_INVALID_PARAM, "matvec error: e_bits outside the rows of the matrix batch");
  // (pair rows of another key are reported in the words of the conversion, as_pair_batch, which this call left the check to)
  static const AggOp op{"matvec", "rows", " and this call indexes its window tables by digits of the plaintext matrix; no masked variant exists",
                        pgpu::matvec_has, "ciphertext batch belongs to a different key"};
  const pgpu_pubkey::PubForm* pf = nullptr;
  RC_TRY(agg_admit(op, key, &x, 1, &pf));
  const int G = pf->H, K = pf->K;
  const size_t LQ = (size_t)2 * G * K, row_bytes = LQ * sizeof(uint32_t);
  const size_t S = policy::matvec_slices(G, rows, cols);
  const int win = policy::matvec_window(rows, cols, e_bits, S, row_bytes);
  AggRun r;
  RC_TRY(r.open(key, pf, x, rows));
  RC_TRY(lanes_order(w, r.x->lane, true));
  // table and partial products: the block arena, on the lane's stream like the operands themselves
  rt::DevMem table, partial;
  RC_TRY(table.alloc(*r.dev, r.s, cols * ((size_t)1 << win) * row_bytes));
  if (S > 1) RC_TRY(partial.alloc(*r.dev, r.s, S * rows * row_bytes));
  pgpu::MatvecArgs a{};
  a.ctx = hensel_pub_view(pf, r.dev->index);
  a.x = r.x->prow(0);
  a.table = (uint32_t*)table.p;
  a.w = w->ptr(0);
  a.w_stride = (size_t)w->words;
  a.w_words = w->words;
  a.e_bits = e_bits;
  a.window = win;
  a.slices = (int)S;
  a.rows = rows;
  a.cols = cols;
  a.out = S > 1 ? (uint32_t*)partial.p : r.o->prow(0);
  RC_TRY(timed_launch(r, cols, G, PGPU_KERNEL_MATVEC, "matvec", [&](unsigned blocks) { return pgpu::launch_matvec_table(G, K, a, blocks, r.s); }));
  RC_TRY(timed_launch(r, rows, G, PGPU_KERNEL_MATVEC, "matvec", [&](unsigned blocks) { return pgpu::launch_matvec(G, K, a, blocks, r.s); }, S));
  // fold the S partial products of every row: ceil(log2 S) element-wise pair products over the slices, in place (slice h + k
  // into slice k; a group reads its two rows before it writes one), the last one into the result batch
  for (size_t cur = S; cur > 1;) {
    const size_t h = (cur + 1) / 2;
    pgpu::PairOpsArgs pa{};
    pa.count = (cur - h) * rows;
    const pgpu_pubkey::PubForm* lf = pair_op_form(key, pf, pa.count);
    pa.ctx = hensel_pub_view(lf, r.dev->index);
    pa.op = pgpu::PO_MUL;
    pa.a = (const uint32_t*)partial.p;
    pa.b = (const uint32_t*)partial.p + h * rows * LQ;
    pa.b_stride = LQ;
    pa.out = h == 1 ? r.o->prow(0) : (uint32_t*)partial.p;
    RC_TRY(pair_op_launch(*r.dev, lf, pa, r.s, PGPU_KERNEL_MATVEC));
    cur = h;
  }
  RC_TRY(lanes_order(w, r.x->lane, false));
  return r.finish(out);
}

// ---- encrypted matrix product (hensel_matmul.hpp; policy.hpp: matmul_*) ----
int pgpu_ct_matmul_plan(int key_bits, size_t n_vec, size_t rows, size_t cols, int e_bits,
                        int* window, int* slices, size_t* tile, size_t* table_bytes, size_t* products) {
  if (key_bits < 1 || n_vec == 0 || rows == 0 || cols == 0 || e_bits < 1)
    return fail(PGPU_ERR_INVALID_PARAM, "matmul plan: key_bits, n_vec, rows, cols and e_bits must be positive");
  int G = 0, K = 0;
  if (!policy::matvec_geometry(key_bits, &G, &K))
    return fail(PGPU_ERR_UNSUPPORTED, "matmul: keys of this size have no pair rows (1024- to 3072-bit key classes only)");
  const size_t row_bytes = (size_t)2 * G * K * sizeof(uint32_t);
  policy::MatmulPlan plan;
  policy::matmul_plan(G, n_vec, rows, cols, e_bits, row_bytes, &plan);
  if (plan.products >= 18446744073709551615.0) return fail(PGPU_ERR_INVALID_PARAM, "matmul plan: the product count overflows");
  if (window) *window = plan.window;
  if (slices) *slices = (int)plan.slices;
  if (tile) *tile = plan.tile;
  if (table_bytes) *table_bytes = plan.tile * cols * ((size_t)1 << plan.window) * row_bytes;
  if (products) *products = (size_t)plan.products;
  return PGPU_OK;
}

int pgpu_batch_ct_matmul(const pgpu_pubkey* key, const pgpu_batch* x, const pgpu_batch* w, size_t n_vec, size_t rows,
                         int e_bits, unsigned flags, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !x || !w || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(x->gen, "batch"));
  RC_TRY(check_gen(w->gen, "batch"));
  if (n_vec == 0 || rows == 0) return fail(PGPU_ERR_INVALID_PARAM, "matmul error: n_vec and rows must be positive");
  if (x->count == 0 || x->count % n_vec != 0) return fail(PGPU_ERR_INVALID_PARAM, "matmul error: n_vec must divide count(x)");
  const size_t cols = x->count / n_vec;
  if (flags & ~PGPU_MATMUL_TRANSPOSED) return fail(PGPU_ERR_INVALID_PARAM, "matmul error: unknown flag bit (PGPU_MATMUL_TRANSPOSED is the only one)");
  if (x->words != 2 * key->n_words) return fail(PGPU_ERR_INVALID_PARAM, "matmul error: ciphertext width mismatch");
  if (w->mont || w->pair_l2) return fail(PGPU_ERR_INVALID_PARAM, "matmul error: the matrix must be a plain uploaded batch");
  if (rows > ~(size_t)0 / cols || w->count != rows * cols)
    return fail(PGPU_ERR_INVALID_PARAM, "matmul error: Size mismatch! (the matrix must hold rows * count(x) / n_vec values)");
  if (e_bits < 1 || e_bits > 64 * w->words) return fail(PGPU_ERR_INVALID_PARAM, "matmul error: e_bits outside the rows of the matrix batch");
  if (rows > ~(size_t)0 / n_vec) return fail(PGPU_ERR_INVALID_PARAM, "matmul error: n_vec * rows overflows");
  // (pair rows of another key are reported in the words of the conversion, as_pair_batch, as for the matvec)
  static const AggOp op{"matmul", "vectors", " and this call indexes its window tables by digits of the plaintext matrix; no masked variant exists",
                        pgpu::matmul_has, "ciphertext batch belongs to a different key"};
  const pgpu_pubkey::PubForm* pf = nullptr;
  RC_TRY(agg_admit(op, key, &x, 1, &pf));
  const int G = pf->H, K = pf->K;
  const size_t LQ = (size_t)2 * G * K, row_bytes = LQ * sizeof(uint32_t);
  const bool tr = (flags & PGPU_MATMUL_TRANSPOSED) != 0;
  policy::MatmulPlan plan;
  policy::matmul_plan(G, n_vec, rows, cols, e_bits, row_bytes, &plan);
  const int win = plan.window;
  const size_t S_max = std::max(plan.slices, plan.last_slices);
  AggRun r;
  RC_TRY(r.open(key, pf, x, n_vec * rows));
  RC_TRY(lanes_order(w, r.x->lane, true));
  // one table block and one partial block for all passes: the block arena, on the lane's stream.  A pass of the transposed
  // layout that is not the whole of x -- its vectors are cols runs of t rows, n_vec rows apart -- goes through a staging
  // block [cols][t], so that the table build walks a contiguous range, and leaves a folded result [rows][t] the same way
  const bool staged = tr && plan.tile < n_vec;
  rt::DevMem table, partial, stage;
  RC_TRY(table.alloc(*r.dev, r.s, plan.tile * cols * ((size_t)1 << win) * row_bytes));
  if (S_max > 1) RC_TRY(partial.alloc(*r.dev, r.s, S_max * plan.tile * rows * row_bytes));
  if (staged) RC_TRY(stage.alloc(*r.dev, r.s, plan.tile * cols * row_bytes));
  for (size_t p = 0; p < plan.passes; ++p) {
    const size_t v0 = p * plan.tile, t = p + 1 == plan.passes ? plan.last : plan.tile, n_out = t * rows;
    const size_t S = p + 1 == plan.passes ? plan.last_slices : plan.slices;
    const uint32_t* xt = tr ? r.x->prow(0) + v0 * LQ : r.x->prow(0) + v0 * cols * LQ;
    uint32_t* dest = tr ? r.o->prow(0) + v0 * LQ : r.o->prow(0) + v0 * rows * LQ;   // (transposed: row i of the tile at dest + i * n_vec rows)
    if (staged) {
      HIP_TRY(hipMemcpy2DAsync(stage.p, t * row_bytes, xt, n_vec * row_bytes, t * row_bytes, cols, hipMemcpyDeviceToDevice, r.s));
      xt = (const uint32_t*)stage.p;
    }
    {
      // the unchanged table build of the matvec over the tile: T[e][d] = x_e^d
      pgpu::MatvecArgs ta{};
      ta.ctx = hensel_pub_view(pf, r.dev->index);
      ta.x = xt;
      ta.table = (uint32_t*)table.p;
      ta.window = win;
      ta.cols = t * cols;
      RC_TRY(timed_launch(r, t * cols, G, PGPU_KERNEL_MATMUL, "matmul", [&](unsigned blocks) { return pgpu::launch_matvec_table(G, K, ta, blocks, r.s); }));
    }
    pgpu::MatmulArgs a{};
    a.ctx = hensel_pub_view(pf, r.dev->index);
    a.table = (const uint32_t*)table.p;
    a.w = w->ptr(0);
    a.w_stride = (size_t)w->words;
    a.w_words = w->words;
    a.e_bits = e_bits;
    a.window = win;
    a.slices = (int)S;
    a.n_out = n_out;
    a.rows = rows;
    a.cols = cols;
    a.t_vec_stride = tr ? 1 : cols;
    a.t_col_stride = tr ? t : 1;
    if (S > 1) {          // partial products [S][t][rows], transposed [S][rows][t]
      a.out = (uint32_t*)partial.p;
      a.o_slice_stride = n_out;
      a.o_vec_stride = tr ? 1 : rows;
      a.o_row_stride = tr ? t : 1;
    } else {              // straight into the result batch
      a.out = dest;
      a.o_slice_stride = 0;
      a.o_vec_stride = tr ? 1 : rows;
      a.o_row_stride = tr ? n_vec : 1;
    }
    RC_TRY(timed_launch(r, n_out, G, PGPU_KERNEL_MATMUL, "matmul", [&](unsigned blocks) { return pgpu::launch_matmul(G, K, a, blocks, r.s); }, S));
    // fold the S partial products of every output as the matvec does: ceil(log2 S) element-wise pair products over the
    // slices, in place, the last one into the result batch where the pass's outputs are contiguous there
    for (size_t cur = S; cur > 1;) {
      const size_t h = (cur + 1) / 2;
      pgpu::PairOpsArgs pa{};
      pa.count = (cur - h) * n_out;
      const pgpu_pubkey::PubForm* lf = pair_op_form(key, pf, pa.count);
      pa.ctx = hensel_pub_view(lf, r.dev->index);
      pa.op = pgpu::PO_MUL;
      pa.a = (const uint32_t*)partial.p;
      pa.b = (const uint32_t*)partial.p + h * n_out * LQ;
      pa.b_stride = LQ;
      pa.out = h == 1 && !staged ? dest : (uint32_t*)partial.p;
      RC_TRY(pair_op_launch(*r.dev, lf, pa, r.s, PGPU_KERNEL_MATMUL));
      cur = h;
    }
    if (S > 1 && staged)
      HIP_TRY(hipMemcpy2DAsync(dest, n_vec * row_bytes, partial.p, t * row_bytes, t * row_bytes, rows, hipMemcpyDeviceToDevice, r.s));
  }
  RC_TRY(lanes_order(w, r.x->lane, false));
  return r.finish(out);
}

// ---- encrypted 2-D convolution (hensel_conv.hpp; policy.hpp: conv_*) ----
static bool conv_dims(const pgpu_conv2d_shape* sh, policy::ConvDims* g) {
  const size_t d[11] = {sh->n_img, sh->c_in, sh->h, sh->w, sh->c_out, sh->kh, sh->kw, sh->stride_h, sh->stride_w, sh->pad_h, sh->pad_w};
  return policy::conv_geometry(d, g);
}
static const char* const kConvShapeMsg =
    ": every dimension and stride must be positive, pad_h < kh, pad_w < kw, kh <= h + 2 pad_h, kw <= w + 2 pad_w, and no size "
    "product may exceed size_t";

int pgpu_ct_conv2d_plan(int key_bits, const pgpu_conv2d_shape* shape, int e_bits, int* window, int* slices, size_t* tile,
                        size_t* table_bytes, size_t* products) {
  if (key_bits < 1 || !shape || e_bits < 1) return fail(PGPU_ERR_INVALID_PARAM, "conv2d plan: key_bits and e_bits must be positive, the shape not null");
  policy::ConvDims g{};
  if (!conv_dims(shape, &g)) return fail(PGPU_ERR_INVALID_PARAM, std::string("conv2d plan") + kConvShapeMsg);
  int G = 0, K = 0;
  if (!policy::matvec_geometry(key_bits, &G, &K))
    return fail(PGPU_ERR_UNSUPPORTED, "conv2d: keys of this size have no pair rows (1024- to 3072-bit key classes only)");
  const size_t row_bytes = (size_t)2 * G * K * sizeof(uint32_t);
  policy::ConvPlan plan;
  policy::conv_plan(G, shape->n_img, g.elems, g.n_o, g.taps, e_bits, row_bytes, &plan);
  if (plan.products >= 18446744073709551615.0) return fail(PGPU_ERR_INVALID_PARAM, "conv2d plan: the product count overflows");
  if (window) *window = plan.window;
  if (slices) *slices = (int)plan.slices;
  if (tile) *tile = plan.tile;
  if (table_bytes) *table_bytes = plan.tile * g.elems * ((size_t)1 << plan.window) * row_bytes;
  if (products) *products = (size_t)plan.products;
  return PGPU_OK;
}

int pgpu_batch_ct_conv2d(const pgpu_pubkey* key, const pgpu_batch* x, const pgpu_batch* w, const pgpu_conv2d_shape* shape,
                         int e_bits, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !x || !w || !shape || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(x->gen, "batch"));
  RC_TRY(check_gen(w->gen, "batch"));
  policy::ConvDims g{};
  if (!conv_dims(shape, &g)) return fail(PGPU_ERR_INVALID_PARAM, std::string("conv2d error") + kConvShapeMsg);
  if (x->count != g.x_count) return fail(PGPU_ERR_INVALID_PARAM, "conv2d error: Size mismatch! (x must hold n_img * c_in * h * w ciphertexts)");
  if (x->words != 2 * key->n_words) return fail(PGPU_ERR_INVALID_PARAM, "conv2d error: ciphertext width mismatch");
  if (w->mont || w->pair_l2) return fail(PGPU_ERR_INVALID_PARAM, "conv2d error: the filters must be a plain uploaded batch");
  if (w->count != g.w_count) return fail(PGPU_ERR_INVALID_PARAM, "conv2d error: Size mismatch! (the filters must hold c_out * c_in * kh * kw values)");
  if (e_bits < 1 || e_bits > 64 * w->words) return fail(PGPU_ERR_INVALID_PARAM, "conv2d error: e_bits outside the rows of the filter batch");
  // (pair rows of another key are reported in the words of the conversion, as_pair_batch, as for the matvec)
  static const AggOp op{"conv2d", "images", " and this call indexes its window tables by digits of the plaintext filters and by positions "
                                            "derived from the shape; no masked variant exists",
                        pgpu::conv_has, "ciphertext batch belongs to a different key"};
  const pgpu_pubkey::PubForm* pf = nullptr;
  RC_TRY(agg_admit(op, key, &x, 1, &pf));
  const int G = pf->H, K = pf->K;
  const size_t LQ = (size_t)2 * G * K, row_bytes = LQ * sizeof(uint32_t);
  policy::ConvPlan plan;
  policy::conv_plan(G, shape->n_img, g.elems, g.n_o, g.taps, e_bits, row_bytes, &plan);
  const int win = plan.window;
  const size_t S_max = std::max(plan.slices, plan.last_slices);
  AggRun r;
  RC_TRY(r.open(key, pf, x, g.out_count));
  RC_TRY(lanes_order(w, r.x->lane, true));
  // one table block and one partial block for all passes: the block arena, on the lane's stream.  The images of a pass
  // and their outputs are contiguous in x and in the result batch
  rt::DevMem table, partial;
  RC_TRY(table.alloc(*r.dev, r.s, plan.tile * g.elems * ((size_t)1 << win) * row_bytes));
  if (S_max > 1) RC_TRY(partial.alloc(*r.dev, r.s, S_max * plan.tile * g.n_o * row_bytes));
  for (size_t p = 0; p < plan.passes; ++p) {
    const size_t i0 = p * plan.tile, t = p + 1 == plan.passes ? plan.last : plan.tile, n_out = t * g.n_o;
    const size_t S = p + 1 == plan.passes ? plan.last_slices : plan.slices;
    uint32_t* dest = r.o->prow(0) + i0 * g.n_o * LQ;
    {
      // the unchanged table build of the matvec over the tile: T[e][d] = x_e^d
      pgpu::MatvecArgs ta{};
      ta.ctx = hensel_pub_view(pf, r.dev->index);
      ta.x = r.x->prow(0) + i0 * g.elems * LQ;
      ta.table = (uint32_t*)table.p;
      ta.window = win;
      ta.cols = t * g.elems;
      RC_TRY(timed_launch(r, t * g.elems, G, PGPU_KERNEL_CONV, "conv2d", [&](unsigned blocks) { return pgpu::launch_matvec_table(G, K, ta, blocks, r.s); }));
    }
    pgpu::ConvArgs a{};
    a.ctx = hensel_pub_view(pf, r.dev->index);
    a.table = (const uint32_t*)table.p;
    a.wt = w->ptr(0);
    a.w_stride = (size_t)w->words;
    a.w_words = w->words;
    a.e_bits = e_bits;
    a.window = win;
    a.slices = (int)S;
    a.n_out = n_out;
    a.c_in = (uint32_t)shape->c_in;       // (conv_geometry: every one of these below 2^31)
    a.h = (uint32_t)shape->h;
    a.w = (uint32_t)shape->w;
    a.c_out = (uint32_t)shape->c_out;
    a.kh = (uint32_t)shape->kh;
    a.kw = (uint32_t)shape->kw;
    // (a stride beyond the padded image leaves one output row or column: any such stride is as good as the smallest one)
    a.sh = (uint32_t)std::min(shape->stride_h, shape->h + 2 * shape->pad_h);
    a.sw = (uint32_t)std::min(shape->stride_w, shape->w + 2 * shape->pad_w);
    a.ph = (uint32_t)shape->pad_h;
    a.pw = (uint32_t)shape->pad_w;
    a.oh = (uint32_t)g.oh;
    a.ow = (uint32_t)g.ow;
    a.out = S > 1 ? (uint32_t*)partial.p : dest;     // partial products [S][t][c_out][oh][ow], or straight into the result batch
    a.o_slice_stride = S > 1 ? n_out : 0;
    RC_TRY(timed_launch(r, n_out, G, PGPU_KERNEL_CONV, "conv2d", [&](unsigned blocks) { return pgpu::launch_conv(G, K, a, blocks, r.s); }, S));
    // fold the S partial products of every output as the matvec does: ceil(log2 S) element-wise pair products over the
    // slices, in place, the last one into the result batch
    for (size_t cur = S; cur > 1;) {
      const size_t h = (cur + 1) / 2;
      pgpu::PairOpsArgs pa{};
      pa.count = (cur - h) * n_out;
      const pgpu_pubkey::PubForm* lf = pair_op_form(key, pf, pa.count);
      pa.ctx = hensel_pub_view(lf, r.dev->index);
      pa.op = pgpu::PO_MUL;
      pa.a = (const uint32_t*)partial.p;
      pa.b = (const uint32_t*)partial.p + h * n_out * LQ;
      pa.b_stride = LQ;
      pa.out = h == 1 ? dest : (uint32_t*)partial.p;
      RC_TRY(pair_op_launch(*r.dev, lf, pa, r.s, PGPU_KERNEL_CONV));
      cur = h;
    }
  }
  RC_TRY(lanes_order(w, r.x->lane, false));
  return r.finish(out);
}

// ---- bucket-method encrypted matvec (hensel_bucket.hpp; policy.hpp: bucket_*) ----
int pgpu_ct_matvec_bucket_plan(int key_bits, size_t rows, size_t cols, int e_bits, int* window, int* block,
                               size_t* bucket_bytes, size_t* products, size_t* depth) {
  if (key_bits < 1 || rows == 0 || cols == 0 || e_bits < 1)
    return fail(PGPU_ERR_INVALID_PARAM, "bucket matvec plan: key_bits, rows, cols and e_bits must be positive");
  int G = 0, K = 0;
  if (!policy::matvec_geometry(key_bits, &G, &K))
    return fail(PGPU_ERR_UNSUPPORTED, "bucket matvec: keys of this size have no pair rows (1024- to 3072-bit key classes only)");
  policy::BucketPlan plan;
  policy::bucket_plan(G, rows, cols, e_bits, (size_t)2 * G * K * sizeof(uint32_t), &plan);
  if (plan.products >= 18446744073709551615.0) return fail(PGPU_ERR_INVALID_PARAM, "bucket matvec plan: the product count overflows");
  if (window) *window = plan.window;
  if (block) *block = plan.block;
  if (bucket_bytes) *bucket_bytes = plan.bucket_bytes;
  if (products) *products = (size_t)plan.products;
  if (depth) *depth = plan.depth;
  return PGPU_OK;
}

int pgpu_batch_ct_matvec_bucket(const pgpu_pubkey* key, const pgpu_batch* x, const uint64_t* w, int w_words, size_t rows,
                                int e_bits, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !x || !w || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(x->gen, "batch"));
  const size_t cols = x->count;
  if (rows == 0) return fail(PGPU_ERR_INVALID_PARAM, "bucket matvec error: rows must be positive");
  if (w_words < 1) return fail(PGPU_ERR_INVALID_PARAM, "bucket matvec error: w_words must be positive");
  if (e_bits < 1 || e_bits > 64 * (long)w_words) return fail(PGPU_ERR_INVALID_PARAM, "bucket matvec error: e_bits outside 1 .. 64 * w_words");
  if (cols == 0) return fail(PGPU_ERR_INVALID_PARAM, "bucket matvec error: empty batch");
  if (x->words != 2 * key->n_words) return fail(PGPU_ERR_INVALID_PARAM, "bucket matvec error: ciphertext width mismatch");
  static const AggOp op{"bucket matvec", "rows", " and this call addresses the ciphertext rows by digits of the plaintext weights; no masked variant exists",
                        pgpu::bucket_has, nullptr};
  const pgpu_pubkey::PubForm* pf = nullptr;
  RC_TRY(agg_admit(op, key, &x, 1, &pf));
  // the plan, on the host: window and block, then the accumulation as a segmented sum over rows * W groups of 2^c buckets
  const int G = pf->H;
  const size_t LQ = (size_t)2 * pf->H * pf->K, row_bytes = LQ * sizeof(uint32_t);
  policy::BucketPlan bp;
  policy::bucket_plan(G, rows, cols, e_bits, row_bytes, &bp);
  const int c = bp.window;
  const size_t W = bp.windows, b = (size_t)bp.block, nb = bp.nb, nseg = (size_t)1 << c;
  // (element numbers are 32-bit entries of the sorted list, bucket and partial-row numbers 31-bit fields of a descriptor)
  constexpr size_t kMax = (size_t)1 << 31;
  if (cols >= kMax || rows >= kMax / W || rows * W >= kMax / cols || rows * W >= kMax / nseg)
    return fail(PGPU_ERR_INVALID_PARAM, "bucket matvec error: rows * windows * count(x) and rows * windows * 2^window must stay below 2^31");
  const size_t groups = rows * W;
  // (a forced window, or the c = 1 that stands in where no window fits the cap, is not held against kMatvecTableCap: this
  // bounds the bucket block on the device and the two counters per bucket of the host's sort before either is allocated)
  if (groups * nseg > policy::kBucketBlockMax / row_bytes)
    return fail(PGPU_ERR_INVALID_PARAM, "bucket matvec error: the bucket block (rows * windows * 2^window pair rows) exceeds 4 GiB");
  std::vector<uint32_t> perm;
  std::vector<size_t> offsets;
  policy::SegsumPlan plan;
  policy::SegsumImage img;
  try {
    policy::bucket_sort(w, w_words, rows, cols, e_bits, c, &perm, &offsets);
    policy::segsum_plan(offsets, policy::segsum_chunk(G, groups * cols), &plan);
    policy::segsum_image(perm, plan, &img);
  } catch (const std::bad_alloc&) {
    return fail(PGPU_ERR_INVALID_PARAM, "bucket matvec error: the sorted column list and its plan do not fit host memory (fewer rows or columns per call)");
  }
  AggRun r;
  RC_TRY(r.open(key, pf, x, rows));
  // buckets [rows][W][2^c], the blocks' U and V [rows][W][nb] each, the windows' S [rows][W]: the block arena, on the lane's stream
  const bool two_levels = b > 1 && nb > 1;
  rt::DevMem dimage, partial, buckets, uv, sw;
  RC_TRY(buckets.alloc(*r.dev, r.s, groups * nseg * row_bytes));
  if (two_levels) RC_TRY(uv.alloc(*r.dev, r.s, 2 * groups * nb * row_bytes));
  if (W > 1) RC_TRY(sw.alloc(*r.dev, r.s, groups * row_bytes));
  if (img.region[0]) RC_TRY(partial.alloc(*r.dev, r.s, (img.region[0] + img.region[1]) * row_bytes));
  RC_TRY(upload_plan_image(*r.dev, r.s, img.image.data(), img.image.size(), &dimage));
  const pgpu_pubkey::PubForm* wide = wide_form(key, pf, pgpu::segsum_wide_has);
  uint32_t* const reg[2] = {(uint32_t*)partial.p, partial.p ? (uint32_t*)partial.p + img.region[0] * LQ : nullptr};
  for (size_t l = 0; l < plan.levels.size(); ++l)
    RC_TRY(segsum_level(r, wide, l == 0 ? r.x->prow(0) : reg[(l - 1) & 1], l == 0 ? (const uint32_t*)dimage.p : nullptr,
                        (const char*)dimage.p + img.level_at[l], plan.levels[l].chunks.size(), (uint32_t*)buckets.p, reg[l & 1],
                        PGPU_KERNEL_BUCKET));
  // the reductions: every launch in the wide form where its chains leave SIMDs empty (policy.hpp: segsum_wide_pays)
  const pgpu_pubkey::PubForm* bwide = wide_form(key, pf, pgpu::bucket_wide_has);
  auto reduce = [&](pgpu::BucketArgs& a) -> int {
    const pgpu_pubkey::PubForm* lf = bwide && policy::segsum_wide_pays(bwide->H, a.chains) ? bwide : pf;
    a.ctx = hensel_pub_view(lf, r.dev->index);
    return timed_launch(r, a.chains, lf->H, PGPU_KERNEL_BUCKET, "bucket matvec",
                        [&](unsigned blocks) { return pgpu::launch_bucket(lf->H, lf->K, a, blocks, r.s); });
  };
  uint32_t* const s_out = W > 1 ? (uint32_t*)sw.p : r.o->prow(0);
  uint32_t* const U = (uint32_t*)uv.p;
  uint32_t* const V = two_levels ? U + groups * nb * LQ : nullptr;
  if (b > 1) {          // level 1: one chain per block (nb == 1: tot is S itself)
    pgpu::BucketArgs a{};
    a.src = (const uint32_t*)buckets.p;
    a.chains = groups * nb;
    a.len = (uint32_t)b;
    a.out_acc = two_levels ? U : nullptr;
    a.out_tot = two_levels ? V : s_out;
    RC_TRY(reduce(a));
  }
  if (nb > 1) {         // level 2: one chain per (row, window) (b == 1: over the buckets themselves, U = B and every V is one)
    pgpu::BucketArgs a{};
    a.src = two_levels ? U : (const uint32_t*)buckets.p;
    a.mul = V;
    a.chains = groups;
    a.len = (uint32_t)nb;
    a.n_sqr = two_levels ? (uint32_t)policy::bucket_log2(b) : 0;
    a.n_mul = two_levels ? (uint32_t)nb : 0;
    a.out_tot = s_out;
    RC_TRY(reduce(a));
  }
  if (W > 1) {          // Horner across the windows: the slot packing's kernel over S as [rows][W], window 0 least significant
    const pgpu_pubkey::PubForm* pwide = wide_form(key, pf, pgpu::pack_wide_has);
    const pgpu_pubkey::PubForm* lf = pwide && policy::segsum_wide_pays(pwide->H, rows) ? pwide : pf;
    pgpu::PackArgs a{};
    a.ctx = hensel_pub_view(lf, r.dev->index);
    a.src = (const uint32_t*)sw.p;
    a.rows = rows;
    a.seg_len = (uint32_t)W;
    a.slot_bits = (uint32_t)c;
    a.out = r.o->prow(0);
    RC_TRY(timed_launch(r, rows, lf->H, PGPU_KERNEL_BUCKET, "bucket matvec", [&](unsigned blocks) { return pgpu::launch_pack(lf->H, lf->K, a, blocks, r.s); }));
  }
  return r.finish(out);
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
  const size_t cols = x->count;
  if (groups == 0 || n_segments == 0) return fail(PGPU_ERR_INVALID_PARAM, "segment sum error: groups and n_segments must be positive");
  if (x->words != 2 * key->n_words) return fail(PGPU_ERR_INVALID_PARAM, "segment sum error: ciphertext width mismatch");
  // (element numbers are 32-bit entries of the sorted list, segment and partial-row numbers 31-bit fields of a descriptor)
  constexpr size_t kMax = (size_t)1 << 31;
  if (cols >= kMax || groups >= kMax / cols || n_segments >= kMax / groups)
    return fail(PGPU_ERR_INVALID_PARAM, "segment sum error: groups * count(x) and groups * n_segments must stay below 2^31");
  static const AggOp op{"segment sum", "segments", " and this call addresses the ciphertext rows by the plaintext segment ids; no masked variant exists",
                        pgpu::matvec_has, nullptr};
  const pgpu_pubkey::PubForm* pf = nullptr;
  RC_TRY(agg_admit(op, key, &x, 1, &pf));
  // the plan, on the host: sorted element numbers, chunk descriptors level by level
  const size_t LQ = (size_t)2 * pf->H * pf->K, row_bytes = LQ * sizeof(uint32_t);
  std::vector<uint32_t> perm;
  std::vector<size_t> offsets;
  if (!policy::segsum_sort(ids, groups, cols, n_segments, &perm, &offsets))
    return fail(PGPU_ERR_INVALID_PARAM, "segment sum error: a segment id is neither below n_segments nor PGPU_SEGMENT_NONE");
  policy::SegsumPlan plan;
  policy::segsum_plan(offsets, policy::segsum_chunk(pf->H, perm.size()), &plan);
  policy::SegsumImage img;
  policy::segsum_image(perm, plan, &img);
  AggRun r;
  RC_TRY(r.open(key, pf, x, groups * n_segments));
  rt::DevMem dimage, partial;
  if (img.region[0]) RC_TRY(partial.alloc(*r.dev, r.s, (img.region[0] + img.region[1]) * row_bytes));
  RC_TRY(upload_plan_image(*r.dev, r.s, img.image.data(), img.image.size(), &dimage));
  const pgpu_pubkey::PubForm* wide = wide_form(key, pf, pgpu::segsum_wide_has);
  uint32_t* const reg[2] = {(uint32_t*)partial.p, partial.p ? (uint32_t*)partial.p + img.region[0] * LQ : nullptr};
  for (size_t l = 0; l < plan.levels.size(); ++l)
    RC_TRY(segsum_level(r, wide, l == 0 ? r.x->prow(0) : reg[(l - 1) & 1], l == 0 ? (const uint32_t*)dimage.p : nullptr,
                        (const char*)dimage.p + img.level_at[l], plan.levels[l].chunks.size(), r.o->prow(0), reg[l & 1], PGPU_KERNEL_SEGSUM));
  return r.finish(out);
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
  const size_t cols = x->count;
  // (CSR positions, rows and chains are 31-bit fields of a descriptor)
  constexpr size_t kMax = (size_t)1 << 31;
  if (rows == 0 || rows >= kMax) return fail(PGPU_ERR_INVALID_PARAM, "spmv error: rows must be positive and below 2^31");
  if (x->words != 2 * key->n_words) return fail(PGPU_ERR_INVALID_PARAM, "spmv error: ciphertext width mismatch");
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
  static const AggOp op{"spmv", "rows", " and this call indexes its window tables by the plaintext column numbers and by digits of the "
                                        "plaintext weights; no masked variant exists",
                        pgpu::spmv_has, nullptr};
  const pgpu_pubkey::PubForm* pf = nullptr;
  RC_TRY(agg_admit(op, key, &x, 1, &pf));
  // the plan, on the host: chain descriptors, then the fold levels over the partial rows
  const int G = pf->H, K = pf->K;
  const size_t LQ = (size_t)2 * G * K, row_bytes = LQ * sizeof(uint32_t);
  policy::SpmvPlan plan;
  if (!policy::spmv_plan(row_ptr, rows, policy::spmv_chunk(G, nnz, rows), &plan))
    return fail(PGPU_ERR_INVALID_PARAM, "spmv error: more chains than a 32-bit descriptor addresses");
  const int win = policy::spmv_window(rows, cols, nnz, plan.n_chains, e_bits, row_bytes);
  policy::SpmvImage img;
  policy::spmv_image(col_idx, nnz, plan, &img);
  AggRun r;
  RC_TRY(r.open(key, pf, x, rows));
  RC_TRY(lanes_order(w, r.x->lane, true));
  rt::DevMem table, dimage, partial;
  RC_TRY(table.alloc(*r.dev, r.s, cols * ((size_t)1 << win) * row_bytes));
  if (img.region[0]) RC_TRY(partial.alloc(*r.dev, r.s, (img.region[0] + img.region[1]) * row_bytes));
  RC_TRY(upload_plan_image(*r.dev, r.s, img.image.data(), img.image.size(), &dimage));
  {
    // the unchanged table build of the matvec: T[j][d] = x[j]^d for every column of x
    pgpu::MatvecArgs ta{};
    ta.ctx = hensel_pub_view(pf, r.dev->index);
    ta.x = r.x->prow(0);
    ta.table = (uint32_t*)table.p;
    ta.window = win;
    ta.cols = cols;
    RC_TRY(timed_launch(r, cols, G, PGPU_KERNEL_SPMV, "spmv", [&](unsigned blocks) { return pgpu::launch_matvec_table(G, K, ta, blocks, r.s); }));
  }
  uint32_t* const reg[2] = {(uint32_t*)partial.p, partial.p ? (uint32_t*)partial.p + img.region[0] * LQ : nullptr};
  {
    pgpu::SpmvArgs a{};
    a.ctx = hensel_pub_view(pf, r.dev->index);
    a.table = (const uint32_t*)table.p;
    a.col_idx = (const uint32_t*)dimage.p;
    a.w = w->ptr(0);
    a.w_stride = (size_t)w->words;
    a.w_words = w->words;
    a.e_bits = e_bits;
    a.window = win;
    a.chunks = (const pgpu::SegsumChunk*)((const char*)dimage.p + img.chains_at);
    a.n_chunks = plan.chains.size();
    a.out = r.o->prow(0);
    a.partial = reg[0];
    RC_TRY(timed_launch(r, a.n_chunks, G, PGPU_KERNEL_SPMV, "spmv", [&](unsigned blocks) { return pgpu::launch_spmv(G, K, a, blocks, r.s); }));
  }
  // the fold levels: the segmented sum's kernel over the partial rows (perm == null)
  const pgpu_pubkey::PubForm* wide = wide_form(key, pf, pgpu::segsum_wide_has);
  for (size_t f = 0; f < plan.fold.levels.size(); ++f)
    RC_TRY(segsum_level(r, wide, reg[f & 1], nullptr, (const char*)dimage.p + img.fold_at[f], plan.fold.levels[f].chunks.size(),
                        r.o->prow(0), reg[(f + 1) & 1], PGPU_KERNEL_SPMV));
  RC_TRY(lanes_order(w, r.x->lane, false));
  return r.finish(out);
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
  for (size_t k = 0; k < n_terms; ++k) {
    if (!xs[k]) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
    RC_TRY(check_gen(xs[k]->gen, "batch"));
  }
  const size_t count = xs[0]->count;
  if (count == 0) return fail(PGPU_ERR_INVALID_PARAM, "weighted sum error: empty batch");
  for (size_t k = 0; k < n_terms; ++k) {   // (batch by batch, its key included: the first batch at fault decides the message)
    if (xs[k]->count != count) return fail(PGPU_ERR_INVALID_PARAM, "weighted sum error: Size mismatch! (every batch must hold count(xs[0]) elements)");
    if (xs[k]->words != 2 * key->n_words) return fail(PGPU_ERR_INVALID_PARAM, "weighted sum error: ciphertext width mismatch");
    if (!same_domain(xs[k]->mont, key->nsq)) return fail(PGPU_ERR_INVALID_PARAM, "weighted sum error: batch belongs to a different key");
  }
  // (the schedule and the row addresses depend on the caller's PLAINTEXT weights only, never on key material or on
  // anything encrypted)
  static const AggOp op{"weighted sum", "elements", "; the schedule and the row addresses depend on the caller's plaintext weights only, but "
                                                    "the aggregation calls on resident ciphertexts have no masked variant",
                        pgpu::matvec_has, nullptr};
  const pgpu_pubkey::PubForm* pf = nullptr;
  RC_TRY(agg_admit(op, key, xs, n_terms, &pf));
  // the schedule, on the host: the slices of the terms, then the fold over their partial rows
  const size_t LQ = (size_t)2 * pf->H * pf->K, row_bytes = LQ * sizeof(uint32_t);
  policy::WsumPlan plan, fold;
  if (!policy::wsum_plan(weights, w_words, n_terms, policy::wsum_slices(pf->H, count, n_terms, !weights), &plan))
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
  AggRun r;
  RC_TRY(r.open_out(key, pf, count, lane));
  for (const auto& kv : pair_of) RC_TRY(lanes_order(kv.second, lane, true));
  rt::DevMem dimage, partial;
  if (S > 1) RC_TRY(partial.alloc(*r.dev, r.s, (S - 1) * count * row_bytes));
  // every entry of the table is addressable: a batch that no step names stands in as the result batch itself
  std::vector<const uint32_t*> tab(n_terms, r.o->prow(0)), ftab;
  for (size_t k = 0; k < n_terms; ++k)
    if (used[k]) tab[k] = pair_of[xs[k]]->prow(0);
  // slice 0 writes the result batch, the others a partial region each; the fold multiplies them into the result batch in
  // place (a group reads row i of every region before it stores row i, and no other live group touches that row)
  for (size_t j = 0; j < S; ++j) {
    plan.slices[j].dst = j == 0 ? r.o->prow(0) : (uint32_t*)partial.p + (j - 1) * count * LQ;
    if (S > 1) ftab.push_back(plan.slices[j].dst);
  }
  if (S > 1) fold.slices[0].dst = r.o->prow(0);
  policy::WsumImage img;
  policy::wsum_image(tab, ftab, plan, fold, &img);
  RC_TRY(upload_plan_image(*r.dev, r.s, img.image.data(), img.image.size(), &dimage));
  const pgpu_pubkey::PubForm* wide = wide_form(key, pf, pgpu::wsum_wide_has);
  auto launch = [&](size_t tab_at, size_t slices_at, size_t steps_at, size_t n_slices) -> int {
    const pgpu_pubkey::PubForm* lf = wide && policy::wsum_wide_pays(wide->H, count * n_slices) ? wide : pf;
    pgpu::WsumArgs a{};
    a.ctx = hensel_pub_view(lf, r.dev->index);
    a.rows = (const uint32_t* const*)((const char*)dimage.p + tab_at);
    a.slices = (const pgpu::WsumSlice*)((const char*)dimage.p + slices_at);
    a.steps = (const pgpu::WsumStep*)((const char*)dimage.p + steps_at);
    a.count = count;
    return timed_launch(r, count, lf->H, PGPU_KERNEL_WSUM, "weighted sum",
                        [&](unsigned blocks) { return pgpu::launch_wsum(lf->H, lf->K, a, blocks, (unsigned)n_slices, r.s); });
  };
  RC_TRY(launch(img.tab_at, img.slices_at, img.steps_at, S));
  if (S > 1) RC_TRY(launch(img.ftab_at, img.fold_slices_at, img.fold_steps_at, 1));
  for (const auto& kv : pair_of) RC_TRY(lanes_order(kv.second, lane, false));
  return r.finish(out);
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
  const size_t count = x->count;
  if (seg_len == 0 || count == 0 || count % seg_len != 0)
    return fail(PGPU_ERR_INVALID_PARAM, "segment scan error: seg_len must be positive and divide count(x)");
  if (flags & ~PGPU_SCAN_REVERSE) return fail(PGPU_ERR_INVALID_PARAM, "segment scan error: unknown flag bit (PGPU_SCAN_REVERSE is the only one)");
  if (x->words != 2 * key->n_words) return fail(PGPU_ERR_INVALID_PARAM, "segment scan error: ciphertext width mismatch");
  // (the address stream here depends on rows, seg_len and the plan alone)
  static const AggOp op{"segment scan", "rows", kNoMaskedVariant, pgpu::matvec_has, nullptr};
  const pgpu_pubkey::PubForm* pf = nullptr;
  RC_TRY(agg_admit(op, key, &x, 1, &pf));
  // the plan, on the host
  const int G = pf->H, K = pf->K;
  const size_t LQ = (size_t)2 * G * K, row_bytes = LQ * sizeof(uint32_t), rows = count / seg_len;
  const int chunk = policy::segscan_chunk(G, rows, seg_len);
  if (!policy::segscan_fits(chunk, rows, seg_len))
    return fail(PGPU_ERR_INVALID_PARAM, "segment scan error: more chunks than a 32-bit carry index addresses (a larger PGPU_SEGSCAN_CHUNK, or fewer rows per call)");
  policy::SegscanPlan plan;
  policy::segscan_plan(rows, seg_len, chunk, (flags & PGPU_SCAN_REVERSE) != 0, &plan);
  policy::SegscanImage img;
  policy::segscan_image(plan, &img);
  const size_t nl = plan.levels.size();
  AggRun r;
  RC_TRY(r.open(key, pf, x, count));
  rt::DevMem dimage, scratch;
  if (img.scratch_rows) RC_TRY(scratch.alloc(*r.dev, r.s, img.scratch_rows * row_bytes));
  RC_TRY(upload_plan_image(*r.dev, r.s, img.image.data(), img.image.size(), &dimage));
  const pgpu_pubkey::PubForm* wide = wide_form(key, pf, pgpu::segsum_wide_has);   // (the up-sweeps: segsum_kernel only)
  uint32_t* const sc = (uint32_t*)scratch.p;
  // level l reads in(l) and writes res(l): x and the result batch, or the totals and the carries of the level above
  auto in = [&](size_t l) -> const uint32_t* { return l == 0 ? r.x->prow(0) : sc + img.totals_at[l - 1] * LQ; };
  auto res = [&](size_t l) -> uint32_t* { return l == 0 ? r.o->prow(0) : sc + img.carry_at[l - 1] * LQ; };
  for (size_t l = 0; l + 1 < nl; ++l)     // up-sweep: the chunk totals, level by level (every descriptor names a row of partial)
    RC_TRY(segsum_level(r, wide, in(l), nullptr, (const char*)dimage.p + img.up_at[l], plan.levels[l].up.size(), nullptr,
                        sc + img.totals_at[l] * LQ, PGPU_KERNEL_SEGSCAN));
  for (size_t l = nl; l-- > 0;) {         // down-sweep: the deepest level has no carries, every other one those below it
    const auto& lv = plan.levels[l];
    pgpu::SegscanArgs a{};
    a.ctx = hensel_pub_view(pf, r.dev->index);
    a.src = in(l);
    a.carry = l + 1 < nl ? res(l + 1) : nullptr;
    a.chunks = (const pgpu::SegscanChunk*)((const char*)dimage.p + img.scan_at[l]);
    a.n_chunks = lv.scan.size();
    a.out = res(l);
    a.step = lv.reverse ? -1 : 1;
    RC_TRY(timed_launch(r, a.n_chunks, G, PGPU_KERNEL_SEGSCAN, "segment scan", [&](unsigned blocks) { return pgpu::launch_segscan(G, K, a, blocks, r.s); }));
  }
  return r.finish(out);
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
  const size_t count = x->count;
  if (seg_len == 0 || count == 0 || count % seg_len != 0)
    return fail(PGPU_ERR_INVALID_PARAM, "pack error: seg_len must be positive and divide count(x)");
  if (slot_bits < 1) return fail(PGPU_ERR_INVALID_PARAM, "pack error: slot_bits must be positive");
  if (!pack_fits(seg_len, slot_bits, key->n.BitSize() - 1))
    return fail(PGPU_ERR_INVALID_PARAM, "pack error: seg_len * slot_bits exceeds bitlen(n) - 1 (the packed plaintext would wrap modulo n)");
  if (x->words != 2 * key->n_words) return fail(PGPU_ERR_INVALID_PARAM, "pack error: ciphertext width mismatch");
  // (the address stream here depends on rows and seg_len alone)
  static const AggOp op{"pack", "rows", kNoMaskedVariant, pgpu::matvec_has, nullptr};
  const pgpu_pubkey::PubForm* pf = nullptr;
  RC_TRY(agg_admit(op, key, &x, 1, &pf));
  const size_t rows = count / seg_len;
  AggRun r;
  RC_TRY(r.open(key, pf, x, rows));
  // (policy.hpp: pack_wide_pays)
  const pgpu_pubkey::PubForm* wide = wide_form(key, pf, pgpu::pack_wide_has);
  const pgpu_pubkey::PubForm* lf = wide && policy::pack_wide_pays(wide->H, rows) ? wide : pf;
  pgpu::PackArgs a{};
  a.ctx = hensel_pub_view(lf, r.dev->index);
  a.src = r.x->prow(0);
  a.rows = rows;
  a.seg_len = (uint32_t)seg_len;     // (both at most bitlen(n) - 1)
  a.slot_bits = (uint32_t)slot_bits;
  a.out = r.o->prow(0);
  RC_TRY(timed_launch(r, rows, lf->H, PGPU_KERNEL_PACK, "pack", [&](unsigned blocks) { return pgpu::launch_pack(lf->H, lf->K, a, blocks, r.s); }));
  return r.finish(out);
}

// ---- ciphertext negation and subtraction (hensel_invert.hpp; policy.hpp: invert_*) ----
int pgpu_ct_negate_plan(int key_bits, size_t count, int* chunk, int* levels, int* launches, size_t* products) {
  if (key_bits < 1 || count == 0) return fail(PGPU_ERR_INVALID_PARAM, "negate plan: key_bits and count must be positive");
  int G = 0, K = 0;
  if (!policy::matvec_geometry(key_bits, &G, &K))
    return fail(PGPU_ERR_UNSUPPORTED, "negate: keys of this size have no pair rows (1024- to 3072-bit key classes only)");
  if (!policy::invert_fits(G, count))
    return fail(PGPU_ERR_INVALID_PARAM, "negate plan: more chains than a 32-bit descriptor field addresses");
  if (chunk) *chunk = policy::invert_chunk(G, count);
  if (levels) *levels = policy::invert_levels(G, count);
  if (launches) *launches = policy::invert_launches(G, count);
  if (products) *products = policy::invert_products(count);
  return PGPU_OK;
}

namespace {
// res[i] = x[i]^-1 mod n^2 (mul != null: mul[i] * x[i]^-1) as a new pair batch of count(x) rows on `lane`; the callers have
// made every check but the plan's.  The one refusal after launches: PGPU_ERR_NOT_INVERTIBLE (nothing is handed out then;
// what was allocated goes back to the lane's arena behind the launches, as after any call)
int invert_batch(const pgpu_pubkey* key, const pgpu_pubkey::PubForm* pf, const char* name, const pgpu_batch* x0,
                 const pgpu_batch* mul0, int lane, std::unique_ptr<pgpu_batch>* res) {
  const size_t count = x0->count;
  const int W = 2 * key->n_words;
  const size_t LQ = (size_t)2 * pf->H * pf->K, row_bytes = LQ * sizeof(uint32_t);
  // the plan, on the host
  if (!policy::invert_fits(pf->H, count))
    return fail(PGPU_ERR_INVALID_PARAM, std::string(name) + " error: more chains than a 32-bit descriptor field addresses (a larger PGPU_INVERT_CHUNK, or fewer elements per call)");
  policy::InvertPlan plan;
  policy::InvertImage img;
  try {
    policy::invert_plan(count, pf->H, &plan);
    policy::invert_image(plan, &img);
  } catch (const std::bad_alloc&) {
    return fail(PGPU_ERR_INVALID_PARAM, std::string(name) + " error: the plan does not fit host memory (fewer elements per call)");
  }
  const size_t nl = plan.levels.size();
  // the operands as pair rows, each converted on its own lane
  std::unique_ptr<pgpu_batch> tx, tm;
  const pgpu_batch *x = nullptr, *mul = nullptr;
  RC_TRY(as_pair_batch(key, x0, &x, &tx));
  if (mul0) RC_TRY(as_pair_batch(key, mul0, &mul, &tm));
  AggRun r;
  RC_TRY(r.open_out(key, pf, count, lane));
  RC_TRY(lanes_order(x, lane, true));
  RC_TRY(lanes_order(mul, lane, true));
  Bounce& bn = bounce();
  RC_TRY(bn.ready());
  // scratch: the levels above the first; io: the inverse of the grand total as a pair row, then the total and its inverse as words
  rt::DevMem dimage, scratch, io;
  if (img.scratch_rows) RC_TRY(scratch.alloc(*r.dev, r.s, img.scratch_rows * row_bytes));
  RC_TRY(io.alloc(*r.dev, r.s, row_bytes + 2 * (size_t)W * sizeof(uint64_t)));
  RC_TRY(upload_plan_image(*r.dev, r.s, img.image.data(), img.image.size(), &dimage));
  const pgpu_pubkey::PubForm* wide = wide_form(key, pf, pgpu::invert_wide_has);
  auto form_of = [&](size_t chains) { return wide && policy::invert_wide_pays(wide->H, chains) ? wide : pf; };
  uint32_t* const sc = (uint32_t*)scratch.p;
  // level l reads in(l) and writes res(l) -- first its running products, then, over them, its inverses
  auto in = [&](size_t l) -> const uint32_t* { return l == 0 ? x->prow(0) : sc + img.in_at[l] * LQ; };
  auto at = [&](size_t l) -> uint32_t* { return l == 0 ? r.o->prow(0) : sc + img.out_at[l] * LQ; };
  for (size_t l = 0; l < nl; ++l) {       // forward: the running products of every chain, level by level
    const auto& lv = plan.levels[l];
    if (l) {
      // the totals of the level below -- the last running product of each of its chains -- side by side: the chains of full
      // length end chunk rows apart, the last one ends with the level
      const size_t below = plan.levels[l - 1].n, c = (size_t)plan.levels[l - 1].chunk, full = below / c;
      uint32_t* dst = sc + img.in_at[l] * LQ;
      if (full)
        HIP_TRY(hipMemcpy2DAsync(dst, row_bytes, at(l - 1) + (c - 1) * LQ, c * row_bytes, row_bytes, full, hipMemcpyDeviceToDevice, r.s));
      if (full < lv.n)
        HIP_TRY(hipMemcpyAsync(dst + full * LQ, at(l - 1) + (below - 1) * LQ, row_bytes, hipMemcpyDeviceToDevice, r.s));
    }
    if (lv.n == 1) break;                 // (count == 1: a chain of one entry has nothing to multiply)
    const pgpu_pubkey::PubForm* lf = form_of(lv.fwd.size());
    pgpu::SegscanArgs a{};
    a.ctx = hensel_pub_view(lf, r.dev->index);
    a.src = in(l);
    a.chunks = (const pgpu::SegscanChunk*)((const char*)dimage.p + img.fwd_at[l]);
    a.n_chunks = lv.fwd.size();
    a.out = at(l);
    a.step = 1;
    RC_TRY(timed_launch(r, a.n_chunks, lf->H, PGPU_KERNEL_INVERT, name, [&](unsigned blocks) { return pgpu::launch_segscan(lf->H, lf->K, a, blocks, r.s); }));
  }
  {
    // the one inversion, on the host: the grand total travels down as the plain value, its inverse up
    const size_t top = plan.levels[nl - 1].n;
    const uint32_t* total = top == 1 ? in(nl - 1) : at(nl - 1) + (top - 1) * LQ;
    uint64_t* const dw = (uint64_t*)((char*)io.p + row_bytes);
    RC_TRY(pair_to_words_on(*r.dev, pf, total, dw, 1, r.s, (size_t)W));
    HIP_TRY(rt::drain_before_copy(r.s));
    HIP_TRY(hipMemcpyAsync(bn.p, dw, (size_t)W * sizeof(uint64_t), hipMemcpyDeviceToHost, r.s));   // (behind the plan upload that read bn.p)
    HIP_TRY(hipStreamSynchronize(r.s));
    bn.pending = false;
    std::vector<uint64_t> inv_words((size_t)W, 0);
    try {
      const BigNumber nsq = key->n * key->n;
      const BigNumber inv = nsq.InverseMul(BigNumber::fromLimbs64((const uint64_t*)bn.p, (size_t)W));
      inv.toLimbs64(inv_words.data(), inv_words.size());
    } catch (const std::runtime_error&) {
      RC_TRY(lanes_order(x, lane, false));
      RC_TRY(lanes_order(mul, lane, false));
      return fail(PGPU_ERR_NOT_INVERTIBLE, std::string(name) + " error: the product of the batch is not a unit modulo n (an element is 0 or shares a factor with n: not a ciphertext)");
    }
    std::memcpy(bn.p, inv_words.data(), (size_t)W * sizeof(uint64_t));
    HIP_TRY(hipMemcpyAsync(dw + W, bn.p, (size_t)W * sizeof(uint64_t), hipMemcpyHostToDevice, r.s));
    HIP_TRY(hipEventRecord(bn.ev, r.s));
    bn.pending = true;
    RC_TRY(words_to_pair_on(*r.dev, pf, dw + W, (size_t)W, W, false, (uint32_t*)io.p, 1, r.s));
  }
  for (size_t l = nl; l-- > 0;) {         // walk back: the top level from the uploaded inverse, every other one from the level above
    const auto& lv = plan.levels[l];
    const pgpu_pubkey::PubForm* lf = form_of(lv.back.size());
    pgpu::InvertArgs a{};
    a.ctx = hensel_pub_view(lf, r.dev->index);
    a.x = in(l);
    a.p = at(l);
    a.u = l + 1 < nl ? at(l + 1) : (const uint32_t*)io.p;
    a.mul = l == 0 && mul ? mul->prow(0) : nullptr;
    a.chunks = (const pgpu::SegscanChunk*)((const char*)dimage.p + img.back_at[l]);
    a.n_chunks = lv.back.size();
    a.out = at(l);
    RC_TRY(timed_launch(r, a.n_chunks, lf->H, PGPU_KERNEL_INVERT, name, [&](unsigned blocks) { return pgpu::launch_invert(lf->H, lf->K, a, blocks, r.s); }));
  }
  RC_TRY(lanes_order(x, lane, false));
  RC_TRY(lanes_order(mul, lane, false));
  *res = std::move(r.o);
  return PGPU_OK;
}
}  // namespace

int pgpu_batch_ct_negate(const pgpu_pubkey* key, const pgpu_batch* x, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !x || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(x->gen, "batch"));
  if (x->words != 2 * key->n_words) return fail(PGPU_ERR_INVALID_PARAM, "negate error: ciphertext width mismatch");
  // (the address stream here depends on count and the plan alone)
  static const AggOp op{"negate", "elements", kNoMaskedVariant, pgpu::invert_has, nullptr};
  const pgpu_pubkey::PubForm* pf = nullptr;
  RC_TRY(agg_admit(op, key, &x, 1, &pf));
  std::unique_ptr<pgpu_batch> o;
  RC_TRY(invert_batch(key, pf, "negate", x, nullptr, x->lane, &o));
  *out = o.release();
  return PGPU_OK;
}

int pgpu_batch_ct_sub(const pgpu_pubkey* key, const pgpu_batch* a, const pgpu_batch* b, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !a || !b || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(a->gen, "batch"));
  RC_TRY(check_gen(b->gen, "batch"));
  const int W = 2 * key->n_words;
  if (a->words != W || b->words != W) return fail(PGPU_ERR_INVALID_PARAM, "CT - CT error: ciphertext width mismatch");
  if (b->count != a->count && b->count != 1) return fail(PGPU_ERR_INVALID_PARAM, "CT - CT error: Size mismatch! (b must hold count(a) elements, or one)");
  static const AggOp op{"CT - CT", "elements", kNoMaskedVariant, pgpu::invert_has, nullptr};
  const pgpu_pubkey::PubForm* pf = nullptr;
  const pgpu_batch* const both[2] = {a, b};
  RC_TRY(agg_admit(op, key, both, 2, &pf));
  std::unique_ptr<pgpu_batch> o;
  if (b->count == a->count) {             // the last walk multiplies a[i] in: no extra launch, no intermediate batch
    RC_TRY(invert_batch(key, pf, "CT - CT", b, a, a->lane, &o));
    *out = o.release();
    return PGPU_OK;
  }
  // broadcast: ONE inverse, multiplied into every a[i] (the element-wise pair product of CT + CT, one shared row)
  std::unique_ptr<pgpu_batch> binv, ta;
  RC_TRY(invert_batch(key, pf, "CT - CT", b, nullptr, a->lane, &binv));
  RC_TRY(as_pair_batch(key, a, &a, &ta));
  AggRun r;
  RC_TRY(r.open_out(key, pf, a->count, a->lane));
  pgpu::PairOpsArgs pa{};
  const pgpu_pubkey::PubForm* lf = pair_op_form(key, pf, a->count);
  pa.ctx = hensel_pub_view(lf, r.dev->index);
  pa.op = pgpu::PO_MUL;
  pa.a = a->prow(0);
  pa.b = binv->prow(0);
  pa.b_stride = 0;
  pa.out = r.o->prow(0);
  pa.count = a->count;
  RC_TRY(pair_op_launch(*r.dev, lf, pa, r.s, PGPU_KERNEL_INVERT));
  return r.finish(out);
}

// ---- signed-weight matvec and matmul (hensel_signed.hpp; policy.hpp: matvec_signed_*, matmul_signed_plan) ----
// The two linear calls above for weights in two's complement: x^-1 by invert_batch (launches of kind PGPU_KERNEL_INVERT, one
// host round trip, the one refusal after launches), a table of 2^w + 1 rows per element over [x ; x^-1], the
// multi-exponentiation on Booth digits, the unchanged fold.  No other route exists: a missing kernel is an error.
int pgpu_ct_matvec_signed_plan(int key_bits, size_t rows, size_t cols, int e_bits, int* window, int* slices, size_t* table_bytes,
                               size_t* products) {
  if (key_bits < 1 || rows == 0 || cols == 0 || e_bits < 1)
    return fail(PGPU_ERR_INVALID_PARAM, "signed matvec plan: key_bits, rows, cols and e_bits must be positive");
  int G = 0, K = 0;
  if (!policy::matvec_geometry(key_bits, &G, &K) || !pgpu::matvec_signed_has(G, K))
    return fail(PGPU_ERR_UNSUPPORTED, "signed matvec: keys of this size have no pair rows (1024- to 3072-bit key classes only)");
  const size_t row_bytes = (size_t)2 * G * K * sizeof(uint32_t);
  const size_t S = policy::matvec_slices(G, rows, cols);
  const int w = policy::matvec_signed_window(rows, cols, e_bits, S, row_bytes);
  const double pr = policy::matvec_signed_products(rows, cols, e_bits, w, S);
  if (pr >= 18446744073709551615.0) return fail(PGPU_ERR_INVALID_PARAM, "signed matvec plan: the product count overflows");
  if (window) *window = w;
  if (slices) *slices = (int)S;
  if (table_bytes) *table_bytes = cols * (((size_t)1 << w) + 1) * row_bytes;
  if (products) *products = (size_t)pr;
  return PGPU_OK;
}

int pgpu_batch_ct_matvec_signed(const pgpu_pubkey* key, const pgpu_batch* x, const pgpu_batch* w, size_t rows, int e_bits,
                                pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !x || !w || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(x->gen, "batch"));
  RC_TRY(check_gen(w->gen, "batch"));
  const size_t cols = x->count;
  if (rows == 0) return fail(PGPU_ERR_INVALID_PARAM, "signed matvec error: rows must be positive");
  if (x->words != 2 * key->n_words) return fail(PGPU_ERR_INVALID_PARAM, "signed matvec error: ciphertext width mismatch");
  if (w->mont || w->pair_l2) return fail(PGPU_ERR_INVALID_PARAM, "signed matvec error: the matrix must be a plain uploaded batch");
  if (rows > ~(size_t)0 / cols || w->count != rows * cols)
    return fail(PGPU_ERR_INVALID_PARAM, "signed matvec error: Size mismatch! (the matrix must hold rows * count(x) values)");
  if (e_bits < 1 || e_bits > 64 * w->words) return fail(PGPU_ERR_INVALID_PARAM, "signed matvec error: e_bits outside the rows of the matrix batch");
  static const AggOp op{"signed matvec", "rows", " and this call indexes its window tables by digits of the plaintext matrix; no masked variant exists",
                        pgpu::matvec_signed_has, "ciphertext batch belongs to a different key"};
  const pgpu_pubkey::PubForm* pf = nullptr;
  RC_TRY(agg_admit(op, key, &x, 1, &pf));
  const int G = pf->H, K = pf->K;
  const size_t LQ = (size_t)2 * G * K, row_bytes = LQ * sizeof(uint32_t);
  const size_t S = policy::matvec_slices(G, rows, cols);
  const int win = policy::matvec_signed_window(rows, cols, e_bits, S, row_bytes);
  // x as pair rows, then its inverses: nothing of this call's own has been launched when the inversion refuses
  std::unique_ptr<pgpu_batch> tx, xinv;
  const pgpu_batch* xp = nullptr;
  RC_TRY(as_pair_batch(key, x, &xp, &tx));
  RC_TRY(invert_batch(key, pf, "signed matvec", xp, nullptr, xp->lane, &xinv));
  AggRun r;
  RC_TRY(r.open(key, pf, xp, rows));
  RC_TRY(lanes_order(w, r.x->lane, true));
  rt::DevMem table, partial;
  RC_TRY(table.alloc(*r.dev, r.s, cols * (((size_t)1 << win) + 1) * row_bytes));
  if (S > 1) RC_TRY(partial.alloc(*r.dev, r.s, S * rows * row_bytes));
  {
    pgpu::SignedTableArgs ta{};
    ta.ctx = hensel_pub_view(pf, r.dev->index);
    ta.x = r.x->prow(0);
    ta.xinv = xinv->prow(0);
    ta.table = (uint32_t*)table.p;
    ta.window = win;
    ta.elems = cols;
    RC_TRY(timed_launch(r, 2 * cols, G, PGPU_KERNEL_MATVEC, "signed matvec", [&](unsigned blocks) { return pgpu::launch_matvec_signed_table(G, K, ta, blocks, r.s); }));
  }
  pgpu::MatvecArgs a{};
  a.ctx = hensel_pub_view(pf, r.dev->index);
  a.x = r.x->prow(0);
  a.table = (uint32_t*)table.p;
  a.w = w->ptr(0);
  a.w_stride = (size_t)w->words;
  a.w_words = w->words;
  a.e_bits = e_bits;
  a.window = win;
  a.slices = (int)S;
  a.rows = rows;
  a.cols = cols;
  a.out = S > 1 ? (uint32_t*)partial.p : r.o->prow(0);
  RC_TRY(timed_launch(r, rows, G, PGPU_KERNEL_MATVEC, "signed matvec", [&](unsigned blocks) { return pgpu::launch_matvec_signed(G, K, a, blocks, r.s); }, S));
  // the fold of pgpu_batch_ct_matvec
  for (size_t cur = S; cur > 1;) {
    const size_t h = (cur + 1) / 2;
    pgpu::PairOpsArgs pa{};
    pa.count = (cur - h) * rows;
    const pgpu_pubkey::PubForm* lf = pair_op_form(key, pf, pa.count);
    pa.ctx = hensel_pub_view(lf, r.dev->index);
    pa.op = pgpu::PO_MUL;
    pa.a = (const uint32_t*)partial.p;
    pa.b = (const uint32_t*)partial.p + h * rows * LQ;
    pa.b_stride = LQ;
    pa.out = h == 1 ? r.o->prow(0) : (uint32_t*)partial.p;
    RC_TRY(pair_op_launch(*r.dev, lf, pa, r.s, PGPU_KERNEL_MATVEC));
    cur = h;
  }
  RC_TRY(lanes_order(w, r.x->lane, false));
  return r.finish(out);
}

int pgpu_ct_matmul_signed_plan(int key_bits, size_t n_vec, size_t rows, size_t cols, int e_bits,
                               int* window, int* slices, size_t* tile, size_t* table_bytes, size_t* products) {
  if (key_bits < 1 || n_vec == 0 || rows == 0 || cols == 0 || e_bits < 1)
    return fail(PGPU_ERR_INVALID_PARAM, "signed matmul plan: key_bits, n_vec, rows, cols and e_bits must be positive");
  int G = 0, K = 0;
  if (!policy::matvec_geometry(key_bits, &G, &K) || !pgpu::matvec_signed_has(G, K))
    return fail(PGPU_ERR_UNSUPPORTED, "signed matmul: keys of this size have no pair rows (1024- to 3072-bit key classes only)");
  if (cols > ~(size_t)0 / n_vec) return fail(PGPU_ERR_INVALID_PARAM, "signed matmul plan: n_vec * cols overflows");
  const size_t row_bytes = (size_t)2 * G * K * sizeof(uint32_t);
  policy::MatmulPlan plan;
  policy::matmul_signed_plan(G, n_vec, rows, cols, e_bits, row_bytes, &plan);
  if (plan.products >= 18446744073709551615.0) return fail(PGPU_ERR_INVALID_PARAM, "signed matmul plan: the product count overflows");
  if (window) *window = plan.window;
  if (slices) *slices = (int)plan.slices;
  if (tile) *tile = plan.tile;
  if (table_bytes) *table_bytes = plan.tile * cols * (((size_t)1 << plan.window) + 1) * row_bytes;
  if (products) *products = (size_t)plan.products;
  return PGPU_OK;
}

int pgpu_batch_ct_matmul_signed(const pgpu_pubkey* key, const pgpu_batch* x, const pgpu_batch* w, size_t n_vec, size_t rows,
                                int e_bits, unsigned flags, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !x || !w || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(x->gen, "batch"));
  RC_TRY(check_gen(w->gen, "batch"));
  if (n_vec == 0 || rows == 0) return fail(PGPU_ERR_INVALID_PARAM, "signed matmul error: n_vec and rows must be positive");
  if (x->count == 0 || x->count % n_vec != 0) return fail(PGPU_ERR_INVALID_PARAM, "signed matmul error: n_vec must divide count(x)");
  const size_t cols = x->count / n_vec;
  if (flags & ~PGPU_MATMUL_TRANSPOSED) return fail(PGPU_ERR_INVALID_PARAM, "signed matmul error: unknown flag bit (PGPU_MATMUL_TRANSPOSED is the only one)");
  if (x->words != 2 * key->n_words) return fail(PGPU_ERR_INVALID_PARAM, "signed matmul error: ciphertext width mismatch");
  if (w->mont || w->pair_l2) return fail(PGPU_ERR_INVALID_PARAM, "signed matmul error: the matrix must be a plain uploaded batch");
  if (rows > ~(size_t)0 / cols || w->count != rows * cols)
    return fail(PGPU_ERR_INVALID_PARAM, "signed matmul error: Size mismatch! (the matrix must hold rows * count(x) / n_vec values)");
  if (e_bits < 1 || e_bits > 64 * w->words) return fail(PGPU_ERR_INVALID_PARAM, "signed matmul error: e_bits outside the rows of the matrix batch");
  if (rows > ~(size_t)0 / n_vec) return fail(PGPU_ERR_INVALID_PARAM, "signed matmul error: n_vec * rows overflows");
  static const AggOp op{"signed matmul", "vectors", " and this call indexes its window tables by digits of the plaintext matrix; no masked variant exists",
                        pgpu::matvec_signed_has, "ciphertext batch belongs to a different key"};
  const pgpu_pubkey::PubForm* pf = nullptr;
  RC_TRY(agg_admit(op, key, &x, 1, &pf));
  const int G = pf->H, K = pf->K;
  const size_t LQ = (size_t)2 * G * K, row_bytes = LQ * sizeof(uint32_t);
  const bool tr = (flags & PGPU_MATMUL_TRANSPOSED) != 0;
  policy::MatmulPlan plan;
  policy::matmul_signed_plan(G, n_vec, rows, cols, e_bits, row_bytes, &plan);
  const int win = plan.window;
  const size_t trows = ((size_t)1 << win) + 1;
  const size_t S_max = std::max(plan.slices, plan.last_slices);
  // x as pair rows, then the inverses of all n_vec * cols elements, once, before the first pass
  std::unique_ptr<pgpu_batch> tx, xinv;
  const pgpu_batch* xp = nullptr;
  RC_TRY(as_pair_batch(key, x, &xp, &tx));
  RC_TRY(invert_batch(key, pf, "signed matmul", xp, nullptr, xp->lane, &xinv));
  AggRun r;
  RC_TRY(r.open(key, pf, xp, n_vec * rows));
  RC_TRY(lanes_order(w, r.x->lane, true));
  // the blocks of pgpu_batch_ct_matmul; a staged pass of the transposed layout stages x^-1 beside x: [2][cols][t]
  const bool staged = tr && plan.tile < n_vec;
  rt::DevMem table, partial, stage;
  RC_TRY(table.alloc(*r.dev, r.s, plan.tile * cols * trows * row_bytes));
  if (S_max > 1) RC_TRY(partial.alloc(*r.dev, r.s, S_max * plan.tile * rows * row_bytes));
  if (staged) RC_TRY(stage.alloc(*r.dev, r.s, 2 * plan.tile * cols * row_bytes));
  for (size_t p = 0; p < plan.passes; ++p) {
    const size_t v0 = p * plan.tile, t = p + 1 == plan.passes ? plan.last : plan.tile, n_out = t * rows;
    const size_t S = p + 1 == plan.passes ? plan.last_slices : plan.slices;
    const size_t x_off = tr ? v0 * LQ : v0 * cols * LQ;
    const uint32_t *xt = r.x->prow(0) + x_off, *xit = xinv->prow(0) + x_off;
    uint32_t* dest = tr ? r.o->prow(0) + v0 * LQ : r.o->prow(0) + v0 * rows * LQ;   // (transposed: row i of the tile at dest + i * n_vec rows)
    if (staged) {
      uint32_t* const s0 = (uint32_t*)stage.p;
      uint32_t* const s1 = s0 + plan.tile * cols * LQ;
      HIP_TRY(hipMemcpy2DAsync(s0, t * row_bytes, xt, n_vec * row_bytes, t * row_bytes, cols, hipMemcpyDeviceToDevice, r.s));
      HIP_TRY(hipMemcpy2DAsync(s1, t * row_bytes, xit, n_vec * row_bytes, t * row_bytes, cols, hipMemcpyDeviceToDevice, r.s));
      xt = s0;
      xit = s1;
    }
    {
      pgpu::SignedTableArgs ta{};
      ta.ctx = hensel_pub_view(pf, r.dev->index);
      ta.x = xt;
      ta.xinv = xit;
      ta.table = (uint32_t*)table.p;
      ta.window = win;
      ta.elems = t * cols;
      RC_TRY(timed_launch(r, 2 * t * cols, G, PGPU_KERNEL_MATMUL, "signed matmul", [&](unsigned blocks) { return pgpu::launch_matvec_signed_table(G, K, ta, blocks, r.s); }));
    }
    pgpu::MatmulArgs a{};
    a.ctx = hensel_pub_view(pf, r.dev->index);
    a.table = (const uint32_t*)table.p;
    a.w = w->ptr(0);
    a.w_stride = (size_t)w->words;
    a.w_words = w->words;
    a.e_bits = e_bits;
    a.window = win;
    a.slices = (int)S;
    a.n_out = n_out;
    a.rows = rows;
    a.cols = cols;
    a.t_vec_stride = tr ? 1 : cols;
    a.t_col_stride = tr ? t : 1;
    if (S > 1) {          // partial products [S][t][rows], transposed [S][rows][t]
      a.out = (uint32_t*)partial.p;
      a.o_slice_stride = n_out;
      a.o_vec_stride = tr ? 1 : rows;
      a.o_row_stride = tr ? t : 1;
    } else {              // straight into the result batch
      a.out = dest;
      a.o_slice_stride = 0;
      a.o_vec_stride = tr ? 1 : rows;
      a.o_row_stride = tr ? n_vec : 1;
    }
    RC_TRY(timed_launch(r, n_out, G, PGPU_KERNEL_MATMUL, "signed matmul", [&](unsigned blocks) { return pgpu::launch_matmul_signed(G, K, a, blocks, r.s); }, S));
    // the fold of pgpu_batch_ct_matmul
    for (size_t cur = S; cur > 1;) {
      const size_t h = (cur + 1) / 2;
      pgpu::PairOpsArgs pa{};
      pa.count = (cur - h) * n_out;
      const pgpu_pubkey::PubForm* lf = pair_op_form(key, pf, pa.count);
      pa.ctx = hensel_pub_view(lf, r.dev->index);
      pa.op = pgpu::PO_MUL;
      pa.a = (const uint32_t*)partial.p;
      pa.b = (const uint32_t*)partial.p + h * n_out * LQ;
      pa.b_stride = LQ;
      pa.out = h == 1 && !staged ? dest : (uint32_t*)partial.p;
      RC_TRY(pair_op_launch(*r.dev, lf, pa, r.s, PGPU_KERNEL_MATMUL));
      cur = h;
    }
    if (S > 1 && staged)
      HIP_TRY(hipMemcpy2DAsync(dest, n_vec * row_bytes, partial.p, t * row_bytes, t * row_bytes, rows, hipMemcpyDeviceToDevice, r.s));
  }
  RC_TRY(lanes_order(w, r.x->lane, false));
  return r.finish(out);
}

// ---- signed-weight convolution and sparse product (hensel_conv_signed.hpp, hensel_spmv_signed.hpp; policy.hpp:
// conv_signed_plan, spmv_signed_*) ----
// pgpu_batch_ct_conv2d / pgpu_batch_ct_spmv for weights in two's complement, after the signed matmul: x^-1 of ALL of x by one
// invert_batch before the first pass (launches of kind PGPU_KERNEL_INVERT, the one refusal after launches), xinv held beside
// x for the call, per pass the signed table over the tile's contiguous range of x and xinv, the multi-exponentiation on
// Booth digits, the unchanged folds.  No other route exists: a missing kernel is an error.
int pgpu_ct_conv2d_signed_plan(int key_bits, const pgpu_conv2d_shape* shape, int e_bits, int* window, int* slices, size_t* tile,
                               size_t* table_bytes, size_t* products) {
  if (key_bits < 1 || !shape || e_bits < 1)
    return fail(PGPU_ERR_INVALID_PARAM, "signed conv2d plan: key_bits and e_bits must be positive, the shape not null");
  policy::ConvDims g{};
  if (!conv_dims(shape, &g)) return fail(PGPU_ERR_INVALID_PARAM, std::string("signed conv2d plan") + kConvShapeMsg);
  int G = 0, K = 0;
  if (!policy::matvec_geometry(key_bits, &G, &K) || !pgpu::conv_signed_has(G, K))
    return fail(PGPU_ERR_UNSUPPORTED, "signed conv2d: keys of this size have no pair rows (1024- to 3072-bit key classes only)");
  const size_t row_bytes = (size_t)2 * G * K * sizeof(uint32_t);
  policy::ConvPlan plan;
  policy::conv_signed_plan(G, shape->n_img, g.elems, g.n_o, g.taps, e_bits, row_bytes, &plan);
  if (plan.products >= 18446744073709551615.0) return fail(PGPU_ERR_INVALID_PARAM, "signed conv2d plan: the product count overflows");
  if (window) *window = plan.window;
  if (slices) *slices = (int)plan.slices;
  if (tile) *tile = plan.tile;
  if (table_bytes) *table_bytes = plan.tile * g.elems * (((size_t)1 << plan.window) + 1) * row_bytes;
  if (products) *products = (size_t)plan.products;
  return PGPU_OK;
}

int pgpu_batch_ct_conv2d_signed(const pgpu_pubkey* key, const pgpu_batch* x, const pgpu_batch* w, const pgpu_conv2d_shape* shape,
                                int e_bits, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !x || !w || !shape || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(x->gen, "batch"));
  RC_TRY(check_gen(w->gen, "batch"));
  policy::ConvDims g{};
  if (!conv_dims(shape, &g)) return fail(PGPU_ERR_INVALID_PARAM, std::string("signed conv2d error") + kConvShapeMsg);
  if (x->count != g.x_count) return fail(PGPU_ERR_INVALID_PARAM, "signed conv2d error: Size mismatch! (x must hold n_img * c_in * h * w ciphertexts)");
  if (x->words != 2 * key->n_words) return fail(PGPU_ERR_INVALID_PARAM, "signed conv2d error: ciphertext width mismatch");
  if (w->mont || w->pair_l2) return fail(PGPU_ERR_INVALID_PARAM, "signed conv2d error: the filters must be a plain uploaded batch");
  if (w->count != g.w_count) return fail(PGPU_ERR_INVALID_PARAM, "signed conv2d error: Size mismatch! (the filters must hold c_out * c_in * kh * kw values)");
  if (e_bits < 1 || e_bits > 64 * w->words) return fail(PGPU_ERR_INVALID_PARAM, "signed conv2d error: e_bits outside the rows of the filter batch");
  static const AggOp op{"signed conv2d", "images", " and this call indexes its window tables by digits of the plaintext filters and by positions "
                                                   "derived from the shape; no masked variant exists",
                        pgpu::conv_signed_has, "ciphertext batch belongs to a different key"};
  const pgpu_pubkey::PubForm* pf = nullptr;
  RC_TRY(agg_admit(op, key, &x, 1, &pf));
  const int G = pf->H, K = pf->K;
  const size_t LQ = (size_t)2 * G * K, row_bytes = LQ * sizeof(uint32_t);
  policy::ConvPlan plan;
  policy::conv_signed_plan(G, shape->n_img, g.elems, g.n_o, g.taps, e_bits, row_bytes, &plan);
  const int win = plan.window;
  const size_t trows = ((size_t)1 << win) + 1;
  const size_t S_max = std::max(plan.slices, plan.last_slices);
  // x as pair rows, then the inverses of all n_img * elems elements, once, before the first pass: nothing of this call's own
  // has been launched when the inversion refuses
  std::unique_ptr<pgpu_batch> tx, xinv;
  const pgpu_batch* xp = nullptr;
  RC_TRY(as_pair_batch(key, x, &xp, &tx));
  RC_TRY(invert_batch(key, pf, "signed conv2d", xp, nullptr, xp->lane, &xinv));
  AggRun r;
  RC_TRY(r.open(key, pf, xp, g.out_count));
  RC_TRY(lanes_order(w, r.x->lane, true));
  // the blocks of pgpu_batch_ct_conv2d, the table one row longer per element
  rt::DevMem table, partial;
  RC_TRY(table.alloc(*r.dev, r.s, plan.tile * g.elems * trows * row_bytes));
  if (S_max > 1) RC_TRY(partial.alloc(*r.dev, r.s, S_max * plan.tile * g.n_o * row_bytes));
  for (size_t p = 0; p < plan.passes; ++p) {
    const size_t i0 = p * plan.tile, t = p + 1 == plan.passes ? plan.last : plan.tile, n_out = t * g.n_o;
    const size_t S = p + 1 == plan.passes ? plan.last_slices : plan.slices;
    uint32_t* dest = r.o->prow(0) + i0 * g.n_o * LQ;
    {
      // the unchanged signed table build over the tile's range of x and xinv
      pgpu::SignedTableArgs ta{};
      ta.ctx = hensel_pub_view(pf, r.dev->index);
      ta.x = r.x->prow(0) + i0 * g.elems * LQ;
      ta.xinv = xinv->prow(0) + i0 * g.elems * LQ;
      ta.table = (uint32_t*)table.p;
      ta.window = win;
      ta.elems = t * g.elems;
      RC_TRY(timed_launch(r, 2 * t * g.elems, G, PGPU_KERNEL_CONV, "signed conv2d", [&](unsigned blocks) { return pgpu::launch_matvec_signed_table(G, K, ta, blocks, r.s); }));
    }
    pgpu::ConvArgs a{};
    a.ctx = hensel_pub_view(pf, r.dev->index);
    a.table = (const uint32_t*)table.p;
    a.wt = w->ptr(0);
    a.w_stride = (size_t)w->words;
    a.w_words = w->words;
    a.e_bits = e_bits;
    a.window = win;
    a.slices = (int)S;
    a.n_out = n_out;
    a.c_in = (uint32_t)shape->c_in;       // (conv_geometry: every one of these below 2^31)
    a.h = (uint32_t)shape->h;
    a.w = (uint32_t)shape->w;
    a.c_out = (uint32_t)shape->c_out;
    a.kh = (uint32_t)shape->kh;
    a.kw = (uint32_t)shape->kw;
    a.sh = (uint32_t)std::min(shape->stride_h, shape->h + 2 * shape->pad_h);
    a.sw = (uint32_t)std::min(shape->stride_w, shape->w + 2 * shape->pad_w);
    a.ph = (uint32_t)shape->pad_h;
    a.pw = (uint32_t)shape->pad_w;
    a.oh = (uint32_t)g.oh;
    a.ow = (uint32_t)g.ow;
    a.out = S > 1 ? (uint32_t*)partial.p : dest;
    a.o_slice_stride = S > 1 ? n_out : 0;
    RC_TRY(timed_launch(r, n_out, G, PGPU_KERNEL_CONV, "signed conv2d", [&](unsigned blocks) { return pgpu::launch_conv_signed(G, K, a, blocks, r.s); }, S));
    // the fold of pgpu_batch_ct_conv2d
    for (size_t cur = S; cur > 1;) {
      const size_t h = (cur + 1) / 2;
      pgpu::PairOpsArgs pa{};
      pa.count = (cur - h) * n_out;
      const pgpu_pubkey::PubForm* lf = pair_op_form(key, pf, pa.count);
      pa.ctx = hensel_pub_view(lf, r.dev->index);
      pa.op = pgpu::PO_MUL;
      pa.a = (const uint32_t*)partial.p;
      pa.b = (const uint32_t*)partial.p + h * n_out * LQ;
      pa.b_stride = LQ;
      pa.out = h == 1 ? dest : (uint32_t*)partial.p;
      RC_TRY(pair_op_launch(*r.dev, lf, pa, r.s, PGPU_KERNEL_CONV));
      cur = h;
    }
  }
  RC_TRY(lanes_order(w, r.x->lane, false));
  return r.finish(out);
}

int pgpu_ct_spmv_signed_plan(int key_bits, size_t rows, size_t cols, size_t nnz, size_t longest_row, int e_bits,
                             int* window, int* chunk, int* levels, size_t* table_bytes, size_t* products) {
  constexpr size_t kMax = (size_t)1 << 31;
  if (key_bits < 1 || rows == 0 || cols == 0 || nnz == 0 || e_bits < 1 || longest_row == 0 || longest_row > nnz ||
      rows >= kMax || nnz >= kMax || (nnz + longest_row - 1) / longest_row > rows)
    return fail(PGPU_ERR_INVALID_PARAM, "signed spmv plan: key_bits, rows, cols, nnz and e_bits must be positive, rows and nnz below 2^31, "
                                        "longest_row between ceil(nnz / rows) and nnz");
  int G = 0, K = 0;
  if (!policy::matvec_geometry(key_bits, &G, &K) || !pgpu::spmv_signed_has(G, K))
    return fail(PGPU_ERR_UNSUPPORTED, "signed spmv: keys of this size have no pair rows (1024- to 3072-bit key classes only)");
  const size_t row_bytes = (size_t)2 * G * K * sizeof(uint32_t);
  const int c = policy::spmv_chunk(G, nnz, rows);
  const size_t chains = policy::spmv_chains_estimate(rows, nnz, longest_row, c);
  const int w = policy::spmv_signed_window(rows, cols, nnz, chains, e_bits, row_bytes);
  if (window) *window = w;
  if (chunk) *chunk = c;
  if (levels) *levels = policy::spmv_levels(c, longest_row);
  if (table_bytes) *table_bytes = cols * (((size_t)1 << w) + 1) * row_bytes;
  if (products) *products = (size_t)policy::spmv_signed_products(rows, cols, nnz, chains, e_bits, w);
  return PGPU_OK;
}

int pgpu_batch_ct_spmv_signed(const pgpu_pubkey* key, const pgpu_batch* x, const uint64_t* row_ptr, const uint32_t* col_idx,
                              const pgpu_batch* w, size_t rows, int e_bits, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!key || !x || !row_ptr || !col_idx || !w || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  RC_TRY(check_gen(key->gen, "key"));
  RC_TRY(check_gen(x->gen, "batch"));
  RC_TRY(check_gen(w->gen, "batch"));
  const size_t cols = x->count;
  // (CSR positions, rows and chains are 31-bit fields of a descriptor)
  constexpr size_t kMax = (size_t)1 << 31;
  if (rows == 0 || rows >= kMax) return fail(PGPU_ERR_INVALID_PARAM, "signed spmv error: rows must be positive and below 2^31");
  if (x->words != 2 * key->n_words) return fail(PGPU_ERR_INVALID_PARAM, "signed spmv error: ciphertext width mismatch");
  if (w->mont || w->pair_l2) return fail(PGPU_ERR_INVALID_PARAM, "signed spmv error: the weights must be a plain uploaded batch");
  if (row_ptr[0] != 0) return fail(PGPU_ERR_INVALID_PARAM, "signed spmv error: row_ptr[0] must be 0");
  for (size_t i = 0; i < rows; ++i)
    if (row_ptr[i + 1] < row_ptr[i]) return fail(PGPU_ERR_INVALID_PARAM, "signed spmv error: row_ptr must be non-decreasing");
  if (row_ptr[rows] == 0) return fail(PGPU_ERR_INVALID_PARAM, "signed spmv error: the matrix has no entries (nnz == 0)");
  if (row_ptr[rows] >= kMax) return fail(PGPU_ERR_INVALID_PARAM, "signed spmv error: nnz must stay below 2^31");
  const size_t nnz = (size_t)row_ptr[rows];
  if (w->count != nnz) return fail(PGPU_ERR_INVALID_PARAM, "signed spmv error: Size mismatch! (the weights must hold row_ptr[rows] values)");
  for (size_t t = 0; t < nnz; ++t)
    if (col_idx[t] >= cols) return fail(PGPU_ERR_INVALID_PARAM, "signed spmv error: a column index is not below count(x)");
  if (e_bits < 1 || e_bits > 64 * w->words) return fail(PGPU_ERR_INVALID_PARAM, "signed spmv error: e_bits outside the rows of the weight batch");
  static const AggOp op{"signed spmv", "rows", " and this call indexes its window tables by the plaintext column numbers and by digits of the "
                                               "plaintext weights; no masked variant exists",
                        pgpu::spmv_signed_has, nullptr};
  const pgpu_pubkey::PubForm* pf = nullptr;
  RC_TRY(agg_admit(op, key, &x, 1, &pf));
  // the plan of pgpu_batch_ct_spmv, on the host; the window held against the signed table
  const int G = pf->H, K = pf->K;
  const size_t LQ = (size_t)2 * G * K, row_bytes = LQ * sizeof(uint32_t);
  policy::SpmvPlan plan;
  if (!policy::spmv_plan(row_ptr, rows, policy::spmv_chunk(G, nnz, rows), &plan))
    return fail(PGPU_ERR_INVALID_PARAM, "signed spmv error: more chains than a 32-bit descriptor addresses");
  const int win = policy::spmv_signed_window(rows, cols, nnz, plan.n_chains, e_bits, row_bytes);
  const size_t trows = ((size_t)1 << win) + 1;
  policy::SpmvImage img;
  policy::spmv_image(col_idx, nnz, plan, &img);
  // x as pair rows, then the inverses of ALL of its elements, referenced by a column index or not: nothing of this call's
  // own has been launched when the inversion refuses
  std::unique_ptr<pgpu_batch> tx, xinv;
  const pgpu_batch* xp = nullptr;
  RC_TRY(as_pair_batch(key, x, &xp, &tx));
  RC_TRY(invert_batch(key, pf, "signed spmv", xp, nullptr, xp->lane, &xinv));
  AggRun r;
  RC_TRY(r.open(key, pf, xp, rows));
  RC_TRY(lanes_order(w, r.x->lane, true));
  rt::DevMem table, dimage, partial;
  RC_TRY(table.alloc(*r.dev, r.s, cols * trows * row_bytes));
  if (img.region[0]) RC_TRY(partial.alloc(*r.dev, r.s, (img.region[0] + img.region[1]) * row_bytes));
  RC_TRY(upload_plan_image(*r.dev, r.s, img.image.data(), img.image.size(), &dimage));
  {
    // the unchanged signed table build over every column of x and xinv
    pgpu::SignedTableArgs ta{};
    ta.ctx = hensel_pub_view(pf, r.dev->index);
    ta.x = r.x->prow(0);
    ta.xinv = xinv->prow(0);
    ta.table = (uint32_t*)table.p;
    ta.window = win;
    ta.elems = cols;
    RC_TRY(timed_launch(r, 2 * cols, G, PGPU_KERNEL_SPMV, "signed spmv", [&](unsigned blocks) { return pgpu::launch_matvec_signed_table(G, K, ta, blocks, r.s); }));
  }
  uint32_t* const reg[2] = {(uint32_t*)partial.p, partial.p ? (uint32_t*)partial.p + img.region[0] * LQ : nullptr};
  {
    pgpu::SpmvArgs a{};
    a.ctx = hensel_pub_view(pf, r.dev->index);
    a.table = (const uint32_t*)table.p;
    a.col_idx = (const uint32_t*)dimage.p;
    a.w = w->ptr(0);
    a.w_stride = (size_t)w->words;
    a.w_words = w->words;
    a.e_bits = e_bits;
    a.window = win;
    a.chunks = (const pgpu::SegsumChunk*)((const char*)dimage.p + img.chains_at);
    a.n_chunks = plan.chains.size();
    a.out = r.o->prow(0);
    a.partial = reg[0];
    RC_TRY(timed_launch(r, a.n_chunks, G, PGPU_KERNEL_SPMV, "signed spmv", [&](unsigned blocks) { return pgpu::launch_spmv_signed(G, K, a, blocks, r.s); }));
  }
  // the fold levels of pgpu_batch_ct_spmv
  const pgpu_pubkey::PubForm* wide = wide_form(key, pf, pgpu::segsum_wide_has);
  for (size_t f = 0; f < plan.fold.levels.size(); ++f)
    RC_TRY(segsum_level(r, wide, reg[f & 1], nullptr, (const char*)dimage.p + img.fold_at[f], plan.fold.levels[f].chunks.size(),
                        r.o->prow(0), reg[(f + 1) & 1], PGPU_KERNEL_SPMV));
  RC_TRY(lanes_order(w, r.x->lane, false));
  return r.finish(out);
}
