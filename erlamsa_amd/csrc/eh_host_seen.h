// eh_host_seen.h - host: the seen set (kernels: eh_seen.h).
#pragma once
static int sn_need(eh_ctx* ctx) {
  if (ctx->sn.have) return EH_OK;
  ctx->err = "no seen set: eh_seen_reserve makes one"; return EH_E_STATE;
}
// Classifies n cases given by their lengths, digests and the filter's results (`lookup`) and / or records the keys of the fresh ones
// (`commit`), then reads the counters back: *fresh / *fresh_bytes = the cases of class 0.  d_status, d_first and d_flag may be null
// (eh_seen.h).  Returns with `st` idle.
static int sn_run(eh_ctx* ctx, const uint64_t* d_len, const int32_t* d_status, const uint64_t* d_digest, const uint64_t* d_first, const uint32_t* d_flag, uint64_t n,
                  bool lookup, bool commit, hipStream_t st, uint64_t* fresh, uint64_t* fresh_bytes) {
  *fresh = *fresh_bytes = 0;
  if (!n) return EH_OK;
  HIPCHK(ctx, ctx->sn.d_cls.grow(n));
  HIPCHK(ctx, ctx->sn.d_pos.grow(n));
  const uint32_t gc = uq_grid(ctx, (n + 63) / 64);
  if (lookup)
    hipLaunchKernelGGL(eh_sn_lookup_kernel, dim3(gc), dim3(64), 0, st, d_len, d_status, d_digest, d_first, n, (const uint64_t*)ctx->sn.d_keys, (const unsigned long long*)ctx->sn.d_tab, ctx->sn.slots,
                       ctx->sn.d_cls);
  hipLaunchKernelGGL(eh_sn_rank_kernel, dim3(1), dim3(64), 0, st, d_len, (const uint8_t*)ctx->sn.d_cls, d_flag, n, ctx->sn.capacity, commit ? 1u : 0u, ctx->sn.d_ctr, ctx->sn.d_pos);
  if (commit) {
    hipLaunchKernelGGL(eh_sn_append_kernel, dim3(gc), dim3(64), 0, st, d_len, d_digest, (const uint64_t*)ctx->sn.d_pos, n, ctx->sn.d_keys);
    hipLaunchKernelGGL(eh_sn_insert_kernel, dim3(gc), dim3(64), 0, st, (const uint64_t*)ctx->sn.d_pos, n, (const uint64_t*)ctx->sn.d_keys, ctx->sn.d_tab, ctx->sn.slots);
  }
  HIPCHK(ctx, hipGetLastError());
  unsigned long long c[4] = {0, 0, 0, 0};
  HIPCHK(ctx, hipStreamSynchronize(st));
  HIPCHK(ctx, hipMemcpy(c, ctx->sn.d_ctr, sizeof(c), hipMemcpyDeviceToHost));
  ctx->sn.held = c[0]; ctx->sn.dropped = c[1]; *fresh = c[2]; *fresh_bytes = c[3];
  return EH_OK;
}
int eh_seen_reserve(eh_ctx* ctx, uint64_t capacity) {
  if (!ctx) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  if (int rc = device_quiet(ctx)) return rc;
  ctx->sn.reset();
  if (!capacity) return EH_OK;
  if (capacity > (1ull << 40)) { ctx->err = "eh_seen_reserve: no memory for a set of that capacity"; return EH_E_NOMEM; }
  uint64_t slots = 2; while (slots < 2 * capacity) slots <<= 1;
  if (ctx->sn.d_keys.reset(2 * capacity) != hipSuccess || ctx->sn.d_tab.reset(slots) != hipSuccess || ctx->sn.d_ctr.reset(4) != hipSuccess) {
    (void)hipGetLastError(); ctx->sn.reset(); ctx->err = "eh_seen_reserve: out of device memory"; return EH_E_NOMEM;
  }
  HIPCHK(ctx, hipMemset(ctx->sn.d_tab, 0xFF, slots * 8));             // every word SN_EMPTY
  HIPCHK(ctx, hipMemset(ctx->sn.d_ctr, 0, 4 * 8));
  HIPCHK(ctx, hipDeviceSynchronize());
  ctx->sn.capacity = capacity; ctx->sn.slots = slots; ctx->sn.have = true;
  return EH_OK;
}
int eh_seen_count(eh_ctx* ctx, uint64_t out[4]) {
  if (!ctx || !out) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock);
  out[0] = ctx->sn.held; out[1] = ctx->sn.capacity; out[2] = ctx->sn.dropped; out[3] = ctx->sn.slots;      // (all 0 without a set)
  return EH_OK;
}
int eh_seen_add_keys(eh_ctx* ctx, const uint64_t* keys, uint64_t m, uint64_t* added) {
  if (!ctx || (!keys && m)) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  if (int rc = sn_need(ctx)) return rc;
  for (uint64_t k = 0; k < m; k++) if (keys[2 * k] >> 63) { ctx->err = "eh_seen_add_keys: a length of 2^63 or more"; return EH_E_INVALID; }
  if (int rc = device_quiet(ctx)) return rc;
  if (added) *added = 0;
  // the first occurrence of every key of the list, in list order: what is left is distinct, as the ranked cases of a batch are
  std::vector<uint64_t> len, dig;
  try {
    std::vector<uint64_t> ix(m);
    for (uint64_t k = 0; k < m; k++) ix[k] = k;
    std::sort(ix.begin(), ix.end(), [&](uint64_t a, uint64_t b) {
      if (keys[2 * a] != keys[2 * b]) return keys[2 * a] < keys[2 * b];
      if (keys[2 * a + 1] != keys[2 * b + 1]) return keys[2 * a + 1] < keys[2 * b + 1];
      return a < b;
    });
    std::vector<uint8_t> firstk(m, 0);
    for (uint64_t k = 0; k < m; k++) firstk[ix[k]] = !k || keys[2 * ix[k]] != keys[2 * ix[k - 1]] || keys[2 * ix[k] + 1] != keys[2 * ix[k - 1] + 1];
    for (uint64_t k = 0; k < m; k++) if (firstk[k]) { len.push_back(keys[2 * k]); dig.push_back(keys[2 * k + 1]); }
  } catch (const std::bad_alloc&) { ctx->err = "out of host memory"; return EH_E_NOMEM; }
  const uint64_t n = len.size();
  if (!n) return EH_OK;
  invalidate_derived(ctx, DERIVED_SEEN);                             // the set changes, and cls / pos: the list's values
  DevBuf<uint64_t> dl, dd;
  HIPCHK(ctx, dl.grow(n));
  HIPCHK(ctx, dd.grow(n));
  HIPCHK(ctx, hipMemcpy(dl, len.data(), n * 8, hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(dd, dig.data(), n * 8, hipMemcpyHostToDevice));
  const uint64_t before = ctx->sn.held;
  uint64_t f, fb;
  int rc = sn_run(ctx, dl, nullptr, dd, nullptr, nullptr, n, true, true, ctx->res.last_stream, &f, &fb); if (rc) return rc;
  if (added) *added = ctx->sn.held - before;
  return EH_OK;
}
int eh_seen_add_corpus(eh_ctx* ctx, uint64_t* added) {
  if (!ctx) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  if (int rc = sn_need(ctx)) return rc;
  if (!ctx->corpus.d) { ctx->err = "no corpus loaded"; return EH_E_STATE; }
  if (int rc = device_quiet(ctx)) return rc;
  if (added) *added = 0;
  const uint64_t n = ctx->corpus.n;
  if (!n) return EH_OK;
  invalidate_derived(ctx, DERIVED_FILTER | DERIVED_SEEN);            // the corpus's values
  DevBuf<uint64_t> dl; DevBuf<int32_t> ds;
  HIPCHK(ctx, dl.grow(n));
  HIPCHK(ctx, ds.grow(n));
  hipStream_t st = ctx->res.last_stream;
  HIPCHK(ctx, hipMemsetAsync(ds, 0, n * 4, st));                      // every entry a candidate (EH_CASE_OK)
  uint64_t* d_len = dl;
  hipLaunchKernelGGL(eh_sn_lens_kernel, dim3(uq_grid(ctx, (n + 63) / 64)), dim3(64), 0, st, (const uint64_t*)ctx->corpus.d_off, d_len, n);
  // the filter first: equal entries add one key, their first's
  int rc = uq_launch(ctx, ctx->corpus.d, ctx->corpus.d_off, dl, ds, n, n + ctx->corpus.bytes / UQ_PIECE + 1, true, true, st); if (rc) return rc;
  const uint64_t before = ctx->sn.held;
  uint64_t f, fb;
  rc = sn_run(ctx, dl, ds, ctx->uq.d_digest, ctx->uq.d_first, ctx->uq.d_flag, n, true, true, st, &f, &fb); if (rc) return rc;
  if (added) *added = ctx->sn.held - before;
  return EH_OK;
}
int eh_seen_export(eh_ctx* ctx, uint64_t* keys, uint64_t cap_keys, uint64_t* n) {
  if (!ctx || (!keys && cap_keys)) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  if (int rc = sn_need(ctx)) return rc;
  if (n) *n = ctx->sn.held;
  const uint64_t m = ctx->sn.held < cap_keys ? ctx->sn.held : cap_keys;
  if (!m) return EH_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpy(keys, ctx->sn.d_keys, m * 16, hipMemcpyDeviceToHost));
  return EH_OK;
}
// The last batch's classes in sn.d_cls and its fresh totals (cached by batch_seq); with `commit` the fresh cases' keys are recorded, once
// per batch.  co_lock held, a set reserved (eh_result_seen, eh_corpus_promote_fresh).
static int sn_result(eh_ctx* ctx, bool commit) {
  int rc = uq_result(ctx, true); if (rc) return rc;                   // digests, first_of and the flags of the last batch (EH_E_STATE before one)
  const uint64_t n = ctx->res.last_n;
  const bool lookup = ctx->sn.seq != ctx->res.batch_seq;
  const bool record = commit && (lookup || !ctx->sn.committed);
  if (lookup || record) {
    uint64_t f, fb;
    rc = sn_run(ctx, ctx->res.d_len, ctx->res.d_status, ctx->uq.d_digest, ctx->uq.d_first, ctx->uq.d_flag, n, lookup, record, ctx->res.last_stream, &f, &fb); if (rc) return rc;
    if (lookup) { ctx->sn.n_fresh = f; ctx->sn.fresh_bytes = fb; ctx->sn.committed = false; }
    if (record) ctx->sn.committed = true;
    ctx->sn.seq = ctx->res.batch_seq;
  }
  return EH_OK;
}
int eh_result_seen(eh_ctx* ctx, uint32_t commit, uint8_t* cls, uint64_t* n_fresh, uint64_t* fresh_bytes) {
  if (!ctx) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  if (int rc = sn_need(ctx)) return rc;
  int rc = sn_result(ctx, commit != 0); if (rc) return rc;
  const uint64_t n = ctx->res.last_n;
  if (cls && n) HIPCHK(ctx, hipMemcpy(cls, ctx->sn.d_cls, n, hipMemcpyDeviceToHost));
  if (n_fresh) *n_fresh = ctx->sn.n_fresh;
  if (fresh_bytes) *fresh_bytes = ctx->sn.fresh_bytes;
  return EH_OK;
}
// Self test hook: the filter's and the set's kernels over a caller-made arena, as eh_selftest_unique; cls (n entries) may be NULL.
int eh_selftest_seen(eh_ctx* ctx, const uint8_t* data, const uint64_t* off, const int32_t* status, uint64_t n, uint32_t commit, uint8_t* cls) {
  if (!ctx) return EH_E_INVALID;
  if (!off || !status || (!data && off[n])) return EH_E_INVALID;
  for (uint64_t i = 0; i < n; i++) if (off[i] > off[i + 1]) { ctx->err = "eh_selftest_seen: offsets must not decrease"; return EH_E_INVALID; }
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  if (int rc = sn_need(ctx)) return rc;
  if (int rc = device_quiet(ctx)) return rc;
  invalidate_derived(ctx, DERIVED_FILTER | DERIVED_SEEN);            // this arena's values
  if (!n) return EH_OK;
  UqArena a;
  int rc = uq_upload_arena(ctx, a, data, off, status, n); if (rc) return rc;
  rc = uq_launch(ctx, a.data, a.off, a.len, a.status, n, a.pieces, true, true, nullptr); if (rc) return rc;
  uint64_t f, fb;
  rc = sn_run(ctx, a.len, a.status, ctx->uq.d_digest, ctx->uq.d_first, ctx->uq.d_flag, n, true, commit != 0, nullptr, &f, &fb); if (rc) return rc;
  if (cls) HIPCHK(ctx, hipMemcpy(cls, ctx->sn.d_cls, n, hipMemcpyDeviceToHost));
  return EH_OK;
}
