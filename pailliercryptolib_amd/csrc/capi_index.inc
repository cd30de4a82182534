// pailliercryptolib_amd -- re-indexing of resident batches: pgpu_batch_gather / _concat / _slice and the plan query
// pgpu_batch_gather_plan (gather.hpp: row_gather_kernel; policy.hpp: gather_*).
// Part of the translation unit of capi.cpp (included there, in place, after capi_aggregate.inc, whose plan upload it
// shares).  The calls take no key and move rows as bytes: every check is made on the host before the first launch or copy.

namespace {
// what the sources of one call have in common: the row size and the domain's row of one
struct IndexRun {
  const pgpu_batch* first = nullptr;
  size_t row_bytes = 0, total = 0;
  std::vector<const pgpu_batch*> distinct;   // every handle once (lane ordering)
};

bool same_index_layout(const pgpu_batch* a, const pgpu_batch* b) {
  if (a->words != b->words || a->pair_l2 != b->pair_l2 || (a->mont != nullptr) != (b->mont != nullptr)) return false;
  if (a->pair_l2) {
    if (!a->pair_form || !b->pair_form) return false;
    if (a->pair_form != b->pair_form && !(a->pair_form->n == b->pair_form->n)) return false;
  }
  if (a->mont && a->mont != b->mont &&
      !(a->mont->geo.L() == b->mont->geo.L() && a->mont->geo.G == b->mont->geo.G && a->mont->N == b->mont->N))
    return false;
  return true;
}

// the checks every call ends with before it touches the device; op: the message prefix
int index_admit(const char* op, const pgpu_batch* const* xs, size_t n_src, IndexRun* run) {
  if (n_src == 0 || n_src > policy::kGatherMaxSources)
    return fail(PGPU_ERR_INVALID_PARAM, std::string(op) + " error: n_src must be between 1 and 65535");
  for (size_t k = 0; k < n_src; ++k) {
    if (!xs[k]) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
    RC_TRY(check_gen(xs[k]->gen, "batch"));
  }
  run->first = xs[0];
  run->row_bytes = (size_t)(xs[0]->pair_l2 ? xs[0]->pair_l2 : xs[0]->words) * 8;
  run->total = 0;
  std::vector<size_t> counts(n_src);
  for (size_t k = 0; k < n_src; ++k) counts[k] = xs[k]->count;
  if (policy::gather_counts_ok(counts.data(), n_src) != n_src)
    return fail(PGPU_ERR_INVALID_PARAM, std::string(op) + " error: a source of 2^32 - 1 rows or more");
  for (size_t k = 0; k < n_src; ++k) {
    if (!same_index_layout(xs[0], xs[k]))
      return fail(PGPU_ERR_INVALID_PARAM, std::string(op) + " error: sources of different layouts (words, domain or key); there is no "
                                                             "conversion inside this call");
    run->total += xs[k]->count;
  }
  run->distinct.assign(xs, xs + n_src);
  std::sort(run->distinct.begin(), run->distinct.end(), std::less<const pgpu_batch*>());
  run->distinct.erase(std::unique(run->distinct.begin(), run->distinct.end()), run->distinct.end());
  if (rt::pool_size() > 1)
    return fail(PGPU_ERR_UNSUPPORTED, std::string(op) + ": pools of more than one GPU are not supported (rows are not sharded yet)");
  return PGPU_OK;
}

// the result batch: what the sources are, on the lane of the first
int index_open(const IndexRun& run, size_t rows, std::unique_ptr<pgpu_batch>* o) {
  const pgpu_batch* x = run.first;
  RC_TRY(new_batch(rows, x->words, o, x->pair_l2, x->lane));
  (*o)->mont = x->mont;
  (*o)->pair_form = x->pair_form;
  return PGPU_OK;
}

// "one" in the sources' domain, as one row
void index_one_row(const pgpu_batch* x, size_t row_bytes, std::vector<char>* row) {
  row->assign(row_bytes, 0);
  if (x->pair_l2) {
    std::memcpy(row->data(), x->pair_form->one_host.data(), std::min(row_bytes, x->pair_form->one_host.size() * sizeof(uint32_t)));
  } else if (x->mont) {
    (pow2(x->mont->geo.rbits()) % x->mont->N).toLimbs64((uint64_t*)row->data(), (size_t)x->words);
  } else {
    (*row)[0] = 1;
  }
}

// one launch of row_gather_kernel over `desc` (sources by their order in `bases`), ordered on the lane of the result
int index_gather(const IndexRun& run, const std::vector<const char*>& bases, const std::vector<pgpu::GatherDesc>& desc,
                 pgpu_batch** out) {
  policy::GatherPlan plan;
  if (!policy::gather_plan(run.row_bytes, desc.size(), &plan)) return fail(PGPU_ERR_INVALID_PARAM, "gather error: row size");
  std::unique_ptr<pgpu_batch> o;
  RC_TRY(index_open(run, desc.size(), &o));
  const int lane = o->lane;
  rt::Device& dev = rt::device(0);
  rt::DeviceGuard g(dev.ordinal);
  hipStream_t s = dev.bs(lane);
  std::vector<char> one;
  index_one_row(run.first, run.row_bytes, &one);
  policy::GatherImage img;
  policy::gather_image(bases, one.data(), run.row_bytes, desc, &img);
  for (const pgpu_batch* x : run.distinct) RC_TRY(lanes_order(x, lane, true));
  rt::DevMem dimage;
  RC_TRY(upload_plan_image(dev, s, img.image.data(), img.image.size(), &dimage));
  pgpu::GatherArgs a{};
  a.bases = (const char* const*)((const char*)dimage.p + img.bases_at);
  a.one = (const char*)dimage.p + img.one_at;
  a.desc = (const pgpu::GatherDesc*)((const char*)dimage.p + img.desc_at);
  a.out = (char*)o->shard[0].p;
  a.n_out = desc.size();
  a.row_bytes = (uint32_t)run.row_bytes;
  a.lanes_log2 = (uint32_t)plan.lanes_log2;
  {
    TimerScope t(dev, s, PGPU_KERNEL_GATHER, PGPU_FORM_FULL_WIDTH);
    if (!pgpu::launch_row_gather(plan.vec_bytes, a, (unsigned)plan.blocks, s))
      return fail(PGPU_ERR_UNSUPPORTED, "gather kernel not compiled for this piece size");
    HIP_TRY(hipGetLastError());
    t.stop();
  }
  for (const pgpu_batch* x : run.distinct) RC_TRY(lanes_order(x, lane, false));
  *out = o.release();
  return PGPU_OK;
}

// stream-ordered device-to-device copies: rows [from, from + rows) of every source in turn, end to end
int index_copy(const IndexRun& run, const pgpu_batch* const* xs, size_t n_src, size_t from, size_t rows, pgpu_batch** out) {
  std::unique_ptr<pgpu_batch> o;
  RC_TRY(index_open(run, rows, &o));
  const int lane = o->lane;
  rt::Device& dev = rt::device(0);
  rt::DeviceGuard g(dev.ordinal);
  hipStream_t s = dev.bs(lane);
  for (const pgpu_batch* x : run.distinct) RC_TRY(lanes_order(x, lane, true));
  char* dst = (char*)o->shard[0].p;
  for (size_t k = 0; k < n_src; ++k) {
    const size_t n = n_src == 1 ? rows : xs[k]->count;
    HIP_TRY(hipMemcpyAsync(dst, (const char*)xs[k]->shard[0].p + from * run.row_bytes, n * run.row_bytes, hipMemcpyDeviceToDevice, s));
    dst += n * run.row_bytes;
  }
  for (const pgpu_batch* x : run.distinct) RC_TRY(lanes_order(x, lane, false));
  *out = o.release();
  return PGPU_OK;
}
}  // namespace

int pgpu_batch_gather_plan(size_t row_bytes, size_t n_out, int* lanes_per_row, int* rows_per_wavefront, int* vec_bytes) {
  policy::GatherPlan plan;
  if (!policy::gather_plan(row_bytes, n_out, &plan))
    return fail(PGPU_ERR_INVALID_PARAM, "gather plan: row_bytes must be a positive multiple of 8 and n_out positive");
  if (lanes_per_row) *lanes_per_row = plan.lanes_per_row;
  if (rows_per_wavefront) *rows_per_wavefront = plan.rows_per_wavefront;
  if (vec_bytes) *vec_bytes = plan.vec_bytes;
  return PGPU_OK;
}

int pgpu_batch_gather(const pgpu_batch* const* xs, size_t n_src, const uint64_t* idx, size_t n_out, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!xs || !idx || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  if (n_out == 0) return fail(PGPU_ERR_INVALID_PARAM, "gather error: n_out must be positive");
  IndexRun run;
  RC_TRY(index_admit("gather", xs, n_src, &run));
  std::vector<size_t> counts(n_src);
  std::vector<const char*> bases(n_src);
  for (size_t k = 0; k < n_src; ++k) {
    counts[k] = xs[k]->count;
    bases[k] = (const char*)xs[k]->shard[0].p;
  }
  std::vector<pgpu::GatherDesc> desc;
  const size_t bad = policy::gather_descs(counts.data(), n_src, idx, n_out, &desc);
  if (bad != n_out)
    return fail(PGPU_ERR_INVALID_PARAM, "gather error: index " + std::to_string(idx[bad]) + " at position " + std::to_string(bad) +
                                            " is beyond the " + std::to_string(run.total) + " rows of the sources");
  return index_gather(run, bases, desc, out);
}

int pgpu_batch_concat(const pgpu_batch* const* xs, size_t n_src, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!xs || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  IndexRun run;
  RC_TRY(index_admit("concat", xs, n_src, &run));
  return index_copy(run, xs, n_src, 0, run.total, out);
}

int pgpu_batch_slice(const pgpu_batch* x, size_t start, size_t count, size_t step, pgpu_batch** out) {
  RC_TRY(rt::check_ready());
  if (!x || !out) return fail(PGPU_ERR_INVALID_PARAM, "null argument");
  if (count == 0) return fail(PGPU_ERR_INVALID_PARAM, "slice error: count must be positive");
  if (step == 0) return fail(PGPU_ERR_INVALID_PARAM, "slice error: step must be positive");
  IndexRun run;
  RC_TRY(index_admit("slice", &x, 1, &run));
  if (start >= x->count || (count - 1) > (x->count - 1 - start) / step)
    return fail(PGPU_ERR_INVALID_PARAM, "slice error: rows " + std::to_string(start) + " + i * " + std::to_string(step) + ", i < " +
                                            std::to_string(count) + ", run past the " + std::to_string(x->count) + " rows of the batch");
  if (step == 1) return index_copy(run, &x, 1, start, count, out);
  std::vector<pgpu::GatherDesc> desc;
  policy::gather_slice_descs(start, count, step, &desc);
  return index_gather(run, {(const char*)x->shard[0].p}, desc, out);
}
