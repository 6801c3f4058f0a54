// eh_host_promote.h - host: corpus promotion (kernels: eh_promote.h) and the download of the corpus as the device holds it.
#pragma once
// The three entry arrays lie one behind the other in pm.d_ent, pm.ent_cap entries each
static uint64_t* pm_ent_src(eh_ctx* ctx) { return ctx->pm.d_ent.p; }
static uint64_t* pm_ent_len(eh_ctx* ctx) { return ctx->pm.d_ent.p + ctx->pm.ent_cap; }
static uint64_t* pm_ent_dst(eh_ctx* ctx) { return ctx->pm.d_ent.p + 2 * ctx->pm.ent_cap; }
// Device arrays for a batch of n_cases cases (0: an explicit list, nothing is selected) and up to m entries
static int pm_ensure(eh_ctx* ctx, uint64_t n_cases, uint64_t m) {
  const uint64_t want = m ? m : 1;
  if (n_cases) HIPCHK(ctx, ctx->pm.d_elen.grow(n_cases));
  if (ctx->pm.ent_cap < want) { ctx->pm.ent_cap = 0; HIPCHK(ctx, ctx->pm.d_ent.reset(3 * want)); ctx->pm.ent_cap = want; }
  HIPCHK(ctx, ctx->pm.d_pfirst.grow(want + 1));
  HIPCHK(ctx, ctx->pm.d_ctr.grow(2));
  return EH_OK;
}
// An explicit list over n cases given on the host (arena offsets, lengths, statuses): checked, then the entry arrays on the device.
static int pm_list(eh_ctx* ctx, const char* who, const uint64_t* idx, uint64_t m, uint64_t n, const uint64_t* off, const uint64_t* len, const int32_t* status, uint64_t* total) {
  *total = 0;
  for (uint64_t k = 0; k < m; k++) if (idx[k] >= n) { ctx->err = std::string(who) + ": list position " + std::to_string(k) + " names case " + std::to_string(idx[k]) + ", outside the batch"; return EH_E_INVALID; }
  for (uint64_t k = 0; k < m; k++) if (status[idx[k]] != EH_CASE_OK) {
    ctx->err = std::string(who) + ": case " + std::to_string(idx[k]) + " (list position " + std::to_string(k) + ") did not end EH_CASE_OK; the corpus is unchanged"; return EH_E_INVALID;
  }
  int rc = pm_ensure(ctx, 0, m); if (rc) return rc;
  if (!m) return EH_OK;
  std::vector<uint64_t> e;
  try { e.resize(3 * m); } catch (const std::bad_alloc&) { ctx->err = "out of host memory"; return EH_E_NOMEM; }
  for (uint64_t k = 0; k < m; k++) { e[k] = off[idx[k]]; e[m + k] = len[idx[k]]; e[2 * m + k] = *total; *total += len[idx[k]]; }
  HIPCHK(ctx, hipMemcpy(pm_ent_src(ctx), e.data(), m * 8, hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(pm_ent_len(ctx), e.data() + m, m * 8, hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(pm_ent_dst(ctx), e.data() + 2 * m, m * 8, hipMemcpyHostToDevice));
  return EH_OK;
}
// The selection on the device: the eligible cases (EH_CASE_OK, class 0 where d_cls is given, 1 <= length <= max_entry) under the budget
// rule, compacted into the entry arrays.  The host reads back the two counters.  Returns with `st` idle.
static int pm_select(eh_ctx* ctx, const int32_t* d_status, const uint8_t* d_cls, const uint64_t* d_len, const uint64_t* d_off, uint64_t n, uint64_t max_entry, uint64_t max_total,
                     hipStream_t st, uint64_t* taken, uint64_t* taken_bytes) {
  *taken = *taken_bytes = 0;
  int rc = pm_ensure(ctx, n, n); if (rc) return rc;
  if (!n) return EH_OK;
  hipLaunchKernelGGL(eh_pm_select_kernel, dim3(uq_grid(ctx, (n + 63) / 64)), dim3(64), 0, st, d_status, d_cls, d_len, n, max_entry, ctx->pm.d_elen.p);
  hipLaunchKernelGGL(eh_pm_scan_kernel, dim3(1), dim3(64), 0, st, (const uint64_t*)ctx->pm.d_elen.p, d_off, n, max_total, ctx->pm.d_ctr.p, pm_ent_src(ctx), pm_ent_len(ctx), pm_ent_dst(ctx));
  HIPCHK(ctx, hipGetLastError());
  unsigned long long c[2] = {0, 0};
  HIPCHK(ctx, hipStreamSynchronize(st));
  HIPCHK(ctx, hipMemcpy(c, ctx->pm.d_ctr, sizeof(c), hipMemcpyDeviceToHost));
  *taken = c[0]; *taken_bytes = c[1];
  return EH_OK;
}
// The m entries the arrays describe (`total` bytes of the arena d_src) become corpus entries: all of the corpus (EH_PROMOTE_REPLACE) or
// behind the entries it has (EH_PROMOTE_APPEND).  In the owned buffers when they have room and nothing they hold must survive elsewhere -
// the steady state of corpus_upload -, otherwise in a new pair with the same room to grow, which is filled completely (an attached or
// too small corpus is copied device to device first) and then adopted: a failure on the way leaves the corpus that was.  The device is
// quiet (device_quiet) and stays so: returns with `st` idle and corpus.h_off equal to the device's offsets.
static int pm_apply(eh_ctx* ctx, const uint8_t* d_src, uint64_t m, uint64_t total, uint32_t mode, hipStream_t st) {
  Corpus& c = ctx->corpus;
  const bool keep = mode == EH_PROMOTE_APPEND && c.d;
  const uint64_t base_n = keep ? c.n : 0, base_bytes = keep ? c.bytes : 0;
  const uint64_t n_after = base_n + m, bytes_after = base_bytes + total;
  const bool owned = c.own.p && c.d == c.own.p && c.d_off == c.own_off.p;
  const bool fits = c.own.p && c.own_off.p && c.own.cap >= bytes_after && c.own_off.cap >= n_after + 1 && (!keep || owned);
  DevBuf<uint8_t> nd; DevBuf<uint64_t> noff;                 // (the corpus in use stays until the new one is complete)
  uint8_t* dd = c.own; uint64_t* doff = c.own_off;
  if (!fits) {
    hipError_t e = nd.grow(bytes_after + bytes_after / 2 + 4096);         // room to grow, as corpus_upload leaves it
    if (e == hipSuccess) e = noff.grow(n_after + n_after / 2 + 16);
    if (e == hipSuccess && base_bytes) e = hipMemcpyAsync(nd, c.d, base_bytes, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && base_n) e = hipMemcpyAsync(noff, c.d_off, base_n * 8, hipMemcpyDeviceToDevice, st);
    HIPCHK(ctx, e);
    dd = nd; doff = noff;
  }
  std::vector<uint64_t> h;
  try { h.resize(n_after + 1); } catch (const std::bad_alloc&) { ctx->err = "out of host memory"; return EH_E_NOMEM; }
  hipLaunchKernelGGL(eh_pm_offsets_kernel, dim3(uq_grid(ctx, (m + 64) / 64)), dim3(64), 0, st, (const uint64_t*)pm_ent_dst(ctx), m, base_n, base_bytes, total, doff);
  if (total) {
    // every piece but an entry's last is full: at most m + total / UQ_PIECE of them
    hipLaunchKernelGGL(eh_uq_scan_kernel, dim3(1), dim3(64), 0, st, (const uint64_t*)pm_ent_len(ctx), ctx->pm.d_pfirst.p, m);
    hipLaunchKernelGGL(eh_pm_copy_kernel, dim3(uq_grid(ctx, m + total / UQ_PIECE)), dim3(64), 0, st, d_src, dd + base_bytes, (const uint64_t*)pm_ent_src(ctx), (const uint64_t*)pm_ent_len(ctx),
                       (const uint64_t*)pm_ent_dst(ctx), (const uint64_t*)ctx->pm.d_pfirst.p, m);
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(st));
  HIPCHK(ctx, hipMemcpy(h.data(), doff, (n_after + 1) * 8, hipMemcpyDeviceToHost));
  if (h[n_after] != bytes_after) { ctx->err = "corpus promotion: the offsets on the device do not end at the arena's size"; return EH_E_HIP; }
  if (fits) { c.d = c.own; c.d_off = c.own_off; c.n = n_after; c.bytes = bytes_after; }
  else adopt_corpus(ctx, nd, noff, n_after, bytes_after);
  c.h_off.swap(h);
  return EH_OK;
}

int eh_corpus_promote(eh_ctx* ctx, const uint64_t* idx, uint64_t m, uint32_t mode, uint64_t* n_after, uint64_t* bytes_after) {
  if (!ctx || (!idx && m) || mode > EH_PROMOTE_APPEND) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  int rc = result_ready(ctx, false); if (rc) return rc;
  rc = device_quiet(ctx); if (rc) return rc;                          // no launch may still read the corpus
  const uint64_t n = ctx->res.last_n;
  std::vector<uint64_t> o, len; std::vector<int32_t> status;
  rc = result_off_len(ctx, &o, len, nullptr); if (rc) return rc;
  try { status.resize(n ? n : 1); } catch (const std::bad_alloc&) { ctx->err = "out of host memory"; return EH_E_NOMEM; }
  if (n) HIPCHK(ctx, hipMemcpy(status.data(), ctx->res.d_status, n * 4, hipMemcpyDeviceToHost));
  uint64_t total = 0;
  rc = pm_list(ctx, "eh_corpus_promote", idx, m, n, o.data(), len.data(), status.data(), &total); if (rc) return rc;
  rc = pm_apply(ctx, ctx->res.d_out, m, total, mode, ctx->res.last_stream); if (rc) return rc;
  if (n_after) *n_after = ctx->corpus.n;
  if (bytes_after) *bytes_after = ctx->corpus.bytes;
  return EH_OK;
}
int eh_corpus_promote_fresh(eh_ctx* ctx, uint64_t max_entry_bytes, uint64_t max_total_bytes, uint32_t mode, uint64_t* taken, uint64_t* taken_bytes) {
  if (!ctx || mode > EH_PROMOTE_APPEND) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  int rc = result_ready(ctx, false); if (rc) return rc;
  rc = sn_need(ctx); if (rc) return rc;
  rc = sn_result(ctx, true); if (rc) return rc;                       // as eh_result_seen(ctx, 1, ...): the batch's classes, its keys recorded once
  rc = device_quiet(ctx); if (rc) return rc;
  uint64_t t = 0, tb = 0;
  rc = pm_select(ctx, ctx->res.d_status, ctx->sn.d_cls, ctx->res.d_len, ctx->res.d_off, ctx->res.last_n, max_entry_bytes, max_total_bytes, ctx->res.last_stream, &t, &tb); if (rc) return rc;
  rc = pm_apply(ctx, ctx->res.d_out, t, tb, mode, ctx->res.last_stream); if (rc) return rc;
  if (taken) *taken = t;
  if (taken_bytes) *taken_bytes = tb;
  return EH_OK;
}
int eh_corpus_download(eh_ctx* ctx, uint8_t* data, uint64_t cap, uint64_t* off, uint64_t cap_entries, uint64_t* n, uint64_t* nbytes) {
  if (!ctx) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  if (!ctx->corpus.d) { ctx->err = "no corpus loaded"; return EH_E_STATE; }
  if (n) *n = ctx->corpus.n;
  if (nbytes) *nbytes = ctx->corpus.bytes;
  if (!data || !off) return EH_OK;                                   // the size query
  if (cap < ctx->corpus.bytes || cap_entries < ctx->corpus.n + 1) { ctx->err = "eh_corpus_download: buffer too small"; return EH_E_INVALID; }
  if (int rc = device_quiet(ctx)) return rc;
  if (ctx->corpus.bytes) HIPCHK(ctx, hipMemcpy(data, ctx->corpus.d, ctx->corpus.bytes, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(off, ctx->corpus.d_off, (ctx->corpus.n + 1) * 8, hipMemcpyDeviceToHost));
  return EH_OK;
}
// Self test hook: the same kernels over a caller-made arena (case i = data[off[i] .. off[i + 1]), status[i]).  cls given: the fresh
// selection with those classes; cls NULL: the list idx[m].  The arena keeps its address modulo 64 on the device (off[0] & 63), so a
// test places sources at any alignment.
int eh_selftest_promote(eh_ctx* ctx, const uint8_t* data, const uint64_t* off, const int32_t* status, const uint8_t* cls, uint64_t n, const uint64_t* idx, uint64_t m,
                        uint64_t max_entry_bytes, uint64_t max_total_bytes, uint32_t mode, uint64_t* taken, uint64_t* taken_bytes) {
  if (!ctx) return EH_E_INVALID;
  if (!off || (!status && n) || (!data && off[n] > off[0]) || (!cls && !idx && m) || mode > EH_PROMOTE_APPEND) return EH_E_INVALID;
  for (uint64_t i = 0; i < n; i++) if (off[i] > off[i + 1]) { ctx->err = "eh_selftest_promote: offsets must not decrease"; return EH_E_INVALID; }
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  if (int rc = device_quiet(ctx)) return rc;
  const uint64_t pad = off[0] & 63, nbytes = off[n] - off[0];
  std::vector<uint64_t> len, rel;
  try { len.resize(n ? n : 1); rel.resize(n ? n : 1); } catch (const std::bad_alloc&) { ctx->err = "out of host memory"; return EH_E_NOMEM; }
  for (uint64_t i = 0; i < n; i++) { len[i] = off[i + 1] - off[i]; rel[i] = off[i] - off[0] + pad; }
  DevBuf<uint8_t> d_data, d_cls; DevBuf<uint64_t> d_off, d_len; DevBuf<int32_t> d_status;
  HIPCHK(ctx, d_data.grow(pad + nbytes + 1));
  if (nbytes) HIPCHK(ctx, hipMemcpy(d_data + pad, data + off[0], nbytes, hipMemcpyHostToDevice));
  uint64_t t = m, tb = 0;
  if (cls) {
    HIPCHK(ctx, d_off.grow(n ? n : 1)); HIPCHK(ctx, d_len.grow(n ? n : 1)); HIPCHK(ctx, d_status.grow(n ? n : 1)); HIPCHK(ctx, d_cls.grow(n ? n : 1));
    if (n) {
      HIPCHK(ctx, hipMemcpy(d_off, rel.data(), n * 8, hipMemcpyHostToDevice));
      HIPCHK(ctx, hipMemcpy(d_len, len.data(), n * 8, hipMemcpyHostToDevice));
      HIPCHK(ctx, hipMemcpy(d_status, status, n * 4, hipMemcpyHostToDevice));
      HIPCHK(ctx, hipMemcpy(d_cls, cls, n, hipMemcpyHostToDevice));
    }
    int rc = pm_select(ctx, d_status, d_cls, d_len, d_off, n, max_entry_bytes, max_total_bytes, nullptr, &t, &tb); if (rc) return rc;
  } else {
    int rc = pm_list(ctx, "eh_selftest_promote", idx, m, n, rel.data(), len.data(), status, &tb); if (rc) return rc;
  }
  int rc = pm_apply(ctx, d_data, t, tb, mode, nullptr); if (rc) return rc;
  if (taken) *taken = t;
  if (taken_bytes) *taken_bytes = tb;
  return EH_OK;
}
