// eh_host_unique.h - host: the uniqueness filter (kernels: eh_unique.h) and the selective download.
#pragma once
static_assert(UQ_PIECE == EH_UNIQUE_PIECE_BYTES, "the header documents the piece size");
static_assert(MAX_PROFILES == EH_MAX_PROFILES && sizeof(ProfileCfg) % 4 == 0, "the header documents the size of the profile table");
// Device buffers for n cases and up to `pieces` pieces; they belong to the context and are reused while they fit.
static int uq_ensure(eh_ctx* ctx, uint64_t n, uint64_t pieces, uint64_t slots) {
  HIPCHK(ctx, ctx->uq.d_digest.grow(n));
  HIPCHK(ctx, ctx->uq.d_first.grow(n));
  HIPCHK(ctx, ctx->uq.d_pfirst.grow(n + 1));
  HIPCHK(ctx, ctx->uq.d_flag.grow(n));
  HIPCHK(ctx, ctx->uq.d_term.grow(pieces));
  HIPCHK(ctx, ctx->uq.d_tab.grow(2 + 2 * slots));
  return EH_OK;
}
static uint32_t uq_grid(const eh_ctx* ctx, uint64_t items) {
  const uint64_t g = (uint64_t)(ctx->cus > 0 ? ctx->cus : 1) * 32u;
  return (uint32_t)(items < 1 ? 1 : items < g ? items : g);
}
// The digest pass (and, with `dedup`, the duplicate pass) over n cases of an arena: launches only, on `st`.  `pieces` bounds the
// piece count (the kernels never write past it).
static int uq_launch(eh_ctx* ctx, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_len, const int32_t* d_status, uint64_t n, uint64_t pieces,
                     bool digest, bool dedup, hipStream_t st) {
  if (!n) return EH_OK;
  uint64_t slots = 64; while (slots < 2 * n) slots <<= 1;
  int rc = uq_ensure(ctx, n, pieces ? pieces : 1, slots); if (rc) return rc;
  if (digest) {
    hipLaunchKernelGGL(eh_uq_scan_kernel, dim3(1), dim3(64), 0, st, d_len, ctx->uq.d_pfirst, n);
    hipLaunchKernelGGL(eh_uq_digest_kernel, dim3(uq_grid(ctx, pieces)), dim3(64), 0, st, d_data, d_off, d_len, (const uint64_t*)ctx->uq.d_pfirst, n, ctx->uq.d_term, pieces);
    hipLaunchKernelGGL(eh_uq_combine_kernel, dim3(uq_grid(ctx, (n + 63) / 64)), dim3(64), 0, st, d_len, (const uint64_t*)ctx->uq.d_pfirst, n, (const unsigned long long*)ctx->uq.d_term, pieces,
                       ctx->uq.d_digest);
  }
  if (dedup) {
    unsigned long long* owner = ctx->uq.d_tab + 2; unsigned long long* rep = owner + slots;
    const uint32_t gc = uq_grid(ctx, (n + 63) / 64);
    hipLaunchKernelGGL(eh_uq_init_kernel, dim3(uq_grid(ctx, (2 + 2 * slots + 63) / 64)), dim3(64), 0, st, ctx->uq.d_tab, 2 + 2 * slots);
    hipLaunchKernelGGL(eh_uq_insert_kernel, dim3(gc), dim3(64), 0, st, d_len, d_status, (const uint64_t*)ctx->uq.d_digest, n, owner, rep, slots, ctx->uq.d_first);
    hipLaunchKernelGGL(eh_uq_resolve_kernel, dim3(gc), dim3(64), 0, st, (const unsigned long long*)rep, n, ctx->uq.d_first, ctx->uq.d_flag);
    hipLaunchKernelGGL(eh_uq_compare_kernel, dim3(uq_grid(ctx, pieces)), dim3(64), 0, st, d_data, d_off, d_len, (const uint64_t*)ctx->uq.d_pfirst, n, (const uint64_t*)ctx->uq.d_first, ctx->uq.d_flag);
    hipLaunchKernelGGL(eh_uq_final_kernel, dim3(gc), dim3(64), 0, st, d_len, d_status, n, ctx->uq.d_first, (const uint32_t*)ctx->uq.d_flag, ctx->uq.d_tab);
  }
  HIPCHK(ctx, hipGetLastError());
  return EH_OK;
}
// the last batch's digests / first_of in the context's device arrays (cached until the next batch)
static int uq_result(eh_ctx* ctx, bool dedup) {
  if (int rc = result_ready(ctx, false)) return rc;                   // (the kernels queue behind the batch on its stream)
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint64_t n = ctx->res.last_n;
  const bool digest = ctx->uq.digest_seq != ctx->res.batch_seq;
  dedup = dedup && ctx->uq.unique_seq != ctx->res.batch_seq;
  if (!digest && !dedup) return EH_OK;
  // every piece but a case's last is full: at most n + arena bytes / UQ_PIECE of them
  const uint64_t arena = ctx->res.d_out.cap > ctx->res.d_out2.cap ? ctx->res.d_out.cap : ctx->res.d_out2.cap;
  int rc = uq_launch(ctx, ctx->res.d_out, ctx->res.d_off, ctx->res.d_len, ctx->res.d_status, n, n + arena / UQ_PIECE + 1, digest, dedup, ctx->res.last_stream);
  if (rc) return rc;
  if (dedup) {
    unsigned long long cnt[2] = {0, 0};
    if (n) { HIPCHK(ctx, hipStreamSynchronize(ctx->res.last_stream)); HIPCHK(ctx, hipMemcpy(cnt, ctx->uq.d_tab, 16, hipMemcpyDeviceToHost)); }
    ctx->uq.n_unique = cnt[0]; ctx->uq.bytes = cnt[1]; ctx->uq.unique_seq = ctx->res.batch_seq;
  }
  ctx->uq.digest_seq = ctx->res.batch_seq;
  return EH_OK;
}
int eh_result_digests(eh_ctx* ctx, uint64_t* digest) {
  if (!ctx) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  int rc = uq_result(ctx, false); if (rc) return rc;
  if (digest && ctx->res.last_n) { HIPCHK(ctx, hipStreamSynchronize(ctx->res.last_stream)); HIPCHK(ctx, hipMemcpy(digest, ctx->uq.d_digest, ctx->res.last_n * 8, hipMemcpyDeviceToHost)); }
  return EH_OK;
}
int eh_result_unique(eh_ctx* ctx, uint64_t* first_of, uint64_t* n_unique, uint64_t* unique_bytes) {
  if (!ctx) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  int rc = uq_result(ctx, true); if (rc) return rc;
  if (first_of && ctx->res.last_n) HIPCHK(ctx, hipMemcpy(first_of, ctx->uq.d_first, ctx->res.last_n * 8, hipMemcpyDeviceToHost));
  if (n_unique) *n_unique = ctx->uq.n_unique;
  if (unique_bytes) *unique_bytes = ctx->uq.bytes;
  return EH_OK;
}
int eh_result_download_select(eh_ctx* ctx, const uint64_t* idx, uint64_t m, uint8_t* data, uint64_t cap, uint64_t* off) {
  if (!ctx || (!idx && m)) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  int rc = result_ready(ctx, false); if (rc) return rc;
  const uint64_t n = ctx->res.last_n;
  for (uint64_t k = 0; k < m; k++) if (idx[k] >= n) { ctx->err = "eh_result_download_select: case index outside the last batch"; return EH_E_INVALID; }
  rc = device_quiet(ctx); if (rc) return rc;
  std::vector<uint64_t> o, len;
  rc = result_off_len(ctx, &o, len, nullptr); if (rc) return rc;
  // the listed cases' offsets and lengths and where each goes, as the m-entry arrays the gather kernel reads: [0, m) offsets, [m, 2m) lengths, [2m, 3m] destinations
  std::vector<uint64_t> sel(3 * m + 1), ord(m + 1);
  uint64_t total = 0, maxlen = 0;
  for (uint64_t k = 0; k < m; k++) { sel[k] = o[idx[k]]; sel[m + k] = len[idx[k]]; ord[k] = total; total += len[idx[k]]; if (len[idx[k]] > maxlen) maxlen = len[idx[k]]; }
  ord[m] = total;
  if (off) for (uint64_t k = 0; k <= m; k++) off[k] = ord[k];
  if (!data || !total) return EH_OK;                                 // (no buffer: off says what is needed)
  if (total > cap) { ctx->err = "eh_result_download_select: buffer too small"; return EH_E_INVALID; }
  for (uint64_t k = 0; k <= m; k++) sel[2 * m + k] = ord[k];
  HIPCHK(ctx, ctx->dl.d_sel.grow(3 * m + 1));
  HIPCHK(ctx, hipMemcpy(ctx->dl.d_sel, sel.data(), (3 * m + 1) * 8, hipMemcpyHostToDevice));
  return gather_download(ctx, data, m, ctx->dl.d_sel, ctx->dl.d_sel + m, ctx->dl.d_sel + 2 * m, ord, maxlen);
}

// A caller-made arena on the device, for the self test hooks: case i = data[off[i] .. off[i + 1]) with status[i]
struct UqArena { DevBuf<uint8_t> data; DevBuf<uint64_t> off, len; DevBuf<int32_t> status; uint64_t pieces = 0; };
static int uq_upload_arena(eh_ctx* ctx, UqArena& a, const uint8_t* data, const uint64_t* off, const int32_t* status, uint64_t n) {
  const uint64_t nbytes = off[n] - off[0];
  std::vector<uint64_t> len(n), rel(n);
  for (uint64_t i = 0; i < n; i++) { len[i] = off[i + 1] - off[i]; rel[i] = off[i] - off[0]; a.pieces += (len[i] + UQ_PIECE - 1) / UQ_PIECE; }
  HIPCHK(ctx, a.data.grow(nbytes ? nbytes : 1));
  HIPCHK(ctx, a.off.grow(n));
  HIPCHK(ctx, a.len.grow(n));
  HIPCHK(ctx, a.status.grow(n));
  if (nbytes) HIPCHK(ctx, hipMemcpy(a.data, data + off[0], nbytes, hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(a.off, rel.data(), n * 8, hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(a.len, len.data(), n * 8, hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(a.status, status, n * 4, hipMemcpyHostToDevice));
  return EH_OK;
}

// Self test hook: the same kernels over a caller-made arena (case i = data[off[i] .. off[i + 1]), status[i]); digest / first_of may be NULL.
int eh_selftest_unique(eh_ctx* ctx, const uint8_t* data, const uint64_t* off, const int32_t* status, uint64_t n, uint64_t* digest, uint64_t* first_of) {
  if (!ctx) return EH_E_INVALID;
  if (!off || !status || (!data && off[n])) return EH_E_INVALID;
  for (uint64_t i = 0; i < n; i++) if (off[i] > off[i + 1]) { ctx->err = "eh_selftest_unique: offsets must not decrease"; return EH_E_INVALID; }
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  if (int rc = device_quiet(ctx)) return rc;
  invalidate_derived(ctx, DERIVED_FILTER);                           // this arena's values
  if (!n) return EH_OK;
  UqArena a;
  int rc = uq_upload_arena(ctx, a, data, off, status, n); if (rc) return rc;
  rc = uq_launch(ctx, a.data, a.off, a.len, a.status, n, a.pieces, true, first_of != nullptr, nullptr);
  if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(nullptr));
  if (digest) HIPCHK(ctx, hipMemcpy(digest, ctx->uq.d_digest, n * 8, hipMemcpyDeviceToHost));
  if (first_of) HIPCHK(ctx, hipMemcpy(first_of, ctx->uq.d_first, n * 8, hipMemcpyDeviceToHost));
  return EH_OK;
}
