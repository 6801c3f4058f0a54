// eh_host_results.h - host: reading the last batch's results.  (The uniqueness filter's and the seen set's: eh_host_unique.h, eh_host_seen.h.)
#pragma once
// The last batch's arena offsets and lengths on the host (n entries each), and the lengths' prefix sums: where each case starts in a
// case-ordered copy (n + 1 entries).  `off` and `ord` may be NULL.
static int result_off_len(eh_ctx* ctx, std::vector<uint64_t>* off, std::vector<uint64_t>& len, std::vector<uint64_t>* ord) {
  const uint64_t n = ctx->res.last_n;
  len.resize(n);
  if (off) off->resize(n);
  if (off && n) HIPCHK(ctx, hipMemcpy(off->data(), ctx->res.d_off, n * 8, hipMemcpyDeviceToHost));
  if (n) HIPCHK(ctx, hipMemcpy(len.data(), ctx->res.d_len, n * 8, hipMemcpyDeviceToHost));
  if (ord) {
    ord->assign(n + 1, 0);
    for (uint64_t i = 0; i < n; i++) (*ord)[i + 1] = (*ord)[i] + len[i];
  }
  return EH_OK;
}
int eh_result_device(eh_ctx* ctx, const uint8_t** d_data, const uint64_t** d_off, const uint64_t** d_len, const int32_t** d_status, uint64_t* total) {
  if (!ctx) return EH_E_INVALID;
  int rc = result_ready(ctx); if (rc) return rc;
  if (d_data) *d_data = ctx->res.d_out;
  if (d_off) *d_off = ctx->res.d_off;
  if (d_len) *d_len = ctx->res.d_len;
  if (d_status) *d_status = ctx->res.d_status;
  if (total) {
    unsigned long long cur = 0;
    if (ctx->res.ordered) HIPCHK(ctx, hipMemcpy(&cur, ctx->res.d_ord + ctx->res.last_n, 8, hipMemcpyDeviceToHost));   // bytes of the compact, case-ordered buffer
    else HIPCHK(ctx, hipMemcpy(&cur, &ctx->res.d_counters.p->out_cursor, 8, hipMemcpyDeviceToHost));         // bump cursor of the completion-ordered arena (16-byte granules)
    *total = cur > ctx->res.d_out.cap ? ctx->res.d_out.cap : cur;               // the cursor runs past the arena after EH_CASE_ARENA_FULL
  }
  return EH_OK;
}

// (no lock, here or in result_download: co_collect calls both after it has released co_lock)
static int result_totals(eh_ctx* ctx, uint64_t* in_bytes, uint64_t* out_bytes, uint64_t* n_cases) {
  int rc = result_ready(ctx); if (rc) return rc;
  if (out_bytes) {
    std::vector<uint64_t> len, ord;
    rc = result_off_len(ctx, nullptr, len, &ord); if (rc) return rc;
    *out_bytes = ord.back();
  }
  if (in_bytes) *in_bytes = ctx->res.last_in_bytes;
  if (n_cases) *n_cases = ctx->res.last_n;
  return EH_OK;
}
int eh_result_totals(eh_ctx* ctx, uint64_t* in_bytes, uint64_t* out_bytes, uint64_t* n_cases) { return ctx ? result_totals(ctx, in_bytes, out_bytes, n_cases) : EH_E_INVALID; }
// The last batch's totals in h_sum, for `who`: the kernel's last workgroup wrote them into page-locked memory, stamped with the
// batch's number, so no copy call is needed - and no runtime call at all for a batch that eh_batch_done has seen end.
static int totals_arrived(eh_ctx* ctx, const char* who, const volatile BatchSummary** hs) {
  if (int rc = result_ready(ctx, false)) return rc;
  if (hipEventQuery(ctx->res.ev1) != hipSuccess) { (void)hipGetLastError(); int rc = eh_sync(ctx); if (rc) return rc; }
  *hs = ctx->res.h_sum;
  if (!*hs || (*hs)->seq != ctx->res.batch_seq) { ctx->err = std::string(who) + ": the batch's totals have not arrived in host memory"; return EH_E_HIP; }
  return EH_OK;
}
// out[0] input bytes, out[1] output bytes, out[2] cases, out[3 + s] cases that ended with status s (0..5) - summed by the kernel,
// one copy of 2 KiB: what a host loop over many small batches reads per batch instead of n lengths and n statuses.
int eh_result_summary(eh_ctx* ctx, uint64_t* out /* 9 values */) {
  if (!ctx || !out) return EH_E_INVALID;
  const volatile BatchSummary* hs = nullptr;
  if (int rc = totals_arrived(ctx, "eh_result_summary", &hs)) return rc;
  out[0] = ctx->res.last_in_bytes; out[1] = hs->out_bytes; out[2] = ctx->res.last_n;
  for (int k = 0; k < 6; k++) out[3 + k] = hs->by_status[k];
  return EH_OK;
}
int eh_result_occupancy(eh_ctx* ctx, uint64_t* out /* 5 values */) {
  if (!ctx || !out) return EH_E_INVALID;
  const volatile BatchSummary* hs = nullptr;
  if (int rc = totals_arrived(ctx, "eh_result_occupancy", &hs)) return rc;
  const bool ran = ctx->res.last_n != 0;                                      // (a batch of no cases ran no mutate kernel)
  out[0] = ran ? hs->wg_ticks : 0; out[1] = ran ? hs->case_ticks : 0; out[2] = ran ? hs->linger_ticks : 0; out[3] = ran ? hs->workgroups : 0;
  out[4] = (uint64_t)ctx->cus * 4u * EH_WAVES_PER_SIMD;
  return EH_OK;
}
// The download pipeline of eh_result_download and eh_result_download_select: item k (a case) is d_soff[k] .. + d_slen[k] of the arena and
// goes to data + ord[k]; d_dst is ord (n + 1 entries) in device memory.  Chunks of consecutive items are gathered on the device into two
// bounce buffers; chunk k goes over PCIe (full rate when `data` is pinned or registered host memory) while chunk k + 1 is gathered.
static int gather_download(eh_ctx* ctx, uint8_t* data, uint64_t n, const uint64_t* d_soff, const uint64_t* d_slen, const uint64_t* d_dst,
                           const std::vector<uint64_t>& ord, uint64_t maxlen) {
  const uint64_t total = ord[n];
  if (total == 0) return EH_OK;
  uint64_t chunk = ctx->dl_chunk < 64 ? 64 : ctx->dl_chunk;        // eh_options.download_chunk_bytes
  uint64_t want = maxlen > chunk ? maxlen : chunk;
  if (want > total) want = total;
  want = (want + 4095) & ~4095ull;
  // (each handle is made once, whichever of them an earlier call got as far as; a stream handle may be NULL where streams are not real)
  if (!ctx->dl.gather) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->dl.gather, hipStreamNonBlocking));
  if (!ctx->dl.copy) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->dl.copy, hipStreamNonBlocking));
  for (int k = 0; k < 2; k++) {
    if (!ctx->dl.ev_g[k]) HIPCHK(ctx, hipEventCreate(&ctx->dl.ev_g[k]));
    if (!ctx->dl.ev_c[k]) HIPCHK(ctx, hipEventCreate(&ctx->dl.ev_c[k]));
  }
  if (ctx->dl.bounce[0].cap < want || ctx->dl.bounce[1].cap < want || ctx->dl.chunk != chunk) {
    ctx->dl.bounce[0].release(); ctx->dl.bounce[1].release();         // both go before either comes back: the new pair may need their room
    for (int k = 0; k < 2; k++) HIPCHK(ctx, ctx->dl.bounce[k].reset(want));
    ctx->dl.chunk = chunk;
  }
  const uint64_t room = ctx->dl.bounce[0].cap;                      // (of either buffer)
  uint64_t a = 0; int k = 0;
  while (a < n) {
    uint64_t b = a + 1;
    while (b < n && ord[b + 1] - ord[a] <= room) b++;
    const int buf = k & 1;
    if (k >= 2) HIPCHK(ctx, hipStreamWaitEvent(ctx->dl.gather, ctx->dl.ev_c[buf], 0));     // the copy that last read this buffer
    uint64_t bytes = ord[b] - ord[a];
    if (bytes) {
      uint64_t cnt = b - a;
      uint32_t g = (uint32_t)ctx->cus * 32u; if (g > cnt) g = (uint32_t)cnt;
      hipLaunchKernelGGL(eh_order_gather_kernel, dim3(g), dim3(64), 0, ctx->dl.gather, (const uint8_t*)ctx->res.d_out, ctx->dl.bounce[buf].p,
                         (const uint64_t*)(d_soff + a), (const uint64_t*)(d_slen + a), (const uint64_t*)(d_dst + a), cnt, ord[a]);
    }
    HIPCHK(ctx, hipEventRecord(ctx->dl.ev_g[buf], ctx->dl.gather));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->dl.copy, ctx->dl.ev_g[buf], 0));
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(data + ord[a], ctx->dl.bounce[buf], bytes, hipMemcpyDeviceToHost, ctx->dl.copy));
    HIPCHK(ctx, hipEventRecord(ctx->dl.ev_c[buf], ctx->dl.copy));
    a = b; k++;
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->dl.copy));
  HIPCHK(ctx, hipGetLastError());
  return EH_OK;
}

static int result_download(eh_ctx* ctx, uint8_t* data, uint64_t cap, uint64_t* off, int32_t* status) {
  int rc = result_ready(ctx); if (rc) return rc;
  const uint64_t n = ctx->res.last_n;
  std::vector<uint64_t> o, len, ord;
  rc = result_off_len(ctx, &o, len, &ord); if (rc) return rc;
  if (status && n) HIPCHK(ctx, hipMemcpy(status, ctx->res.d_status, n * 4, hipMemcpyDeviceToHost));
  const uint64_t total = ord[n];
  if (off) memcpy(off, ord.data(), (n + 1) * 8);
  if (data) {
    if (total > cap) { ctx->err = "download buffer too small"; return EH_E_INVALID; }
    if (ctx->res.ordered) {                                          // already in case order and contiguous: one copy
      if (total) HIPCHK(ctx, hipMemcpy(data, ctx->res.d_out, total, hipMemcpyDeviceToHost));
      return EH_OK;
    }
    // completion-ordered arena -> case order (gather_download)
    if (total == 0) return EH_OK;
    uint64_t maxlen = 0; for (uint64_t i = 0; i < n; i++) if (len[i] > maxlen) maxlen = len[i];
    HIPCHK(ctx, ctx->res.d_ord.grow(n + 1));
    HIPCHK(ctx, hipMemcpy(ctx->res.d_ord, ord.data(), (n + 1) * 8, hipMemcpyHostToDevice));
    return gather_download(ctx, data, n, ctx->res.d_off, ctx->res.d_len, ctx->res.d_ord, ord, maxlen);
  }
  return EH_OK;
}

int eh_result_download(eh_ctx* ctx, uint8_t* data, uint64_t cap, uint64_t* off, int32_t* status) { return ctx ? result_download(ctx, data, cap, off, status) : EH_E_INVALID; }

// erlamsa_out:file_writer/1 (erlamsa_out.erl:103-123): Tokens = re:split(Str, "%n"), Filename = the tokens joined by
// integer_to_list(N) (build_name/3) — every "%n" of the template becomes the case number.
static std::string build_name(const std::string& tmpl, uint64_t n) {
  const std::string num = std::to_string(n);
  std::string out; size_t pos = 0;
  for (;;) {
    size_t e = tmpl.find("%n", pos);
    if (e == std::string::npos) { out.append(tmpl, pos, std::string::npos); break; }
    out.append(tmpl, pos, e - pos); out += num; pos = e + 2;
  }
  return out;
}
int eh_result_write_files(eh_ctx* ctx, const char* name_template, uint64_t first_number, uint32_t threads, uint64_t* files_written, uint64_t* bytes_written, uint64_t* not_written) {
  if (!ctx || !name_template) return EH_E_INVALID;
  uint64_t in_b = 0, total = 0, n = 0;
  int rc = result_totals(ctx, &in_b, &total, &n);                        // (result_ready first)
  if (rc) return rc;
  // one case-ordered download (device gather + overlapped copies), then the files are written by a few host threads
  std::vector<uint64_t> off(n + 1); std::vector<int32_t> st(n ? n : 1);
  uint8_t* host = nullptr;
  bool pinned = total > 0 && hipHostMalloc((void**)&host, total, 0) == hipSuccess;
  if (total > 0 && !pinned) { host = (uint8_t*)malloc(total); if (!host) { ctx->err = "eh_result_write_files: out of host memory"; return EH_E_NOMEM; } }
  rc = result_download(ctx, host, total, off.data(), st.data());
  std::atomic<uint64_t> next{0}, files{0}, bytes{0}, skipped{0}; std::atomic<int> failed{0};
  std::string first_error;
  std::mutex err_lock;
  if (!rc) {
    const std::string tmpl(name_template);
    auto work = [&]() {
      for (;;) {
        uint64_t i = next.fetch_add(1);
        if (i >= n || failed.load()) return;
        // the reference opens the file inside the worker, after the mutation: a case whose worker died or was killed
        // (statuses 1, 5) or that stopped at an engine limit (2, 3, 4) leaves no file
        if (st[i] != EH_CASE_OK) { skipped++; continue; }
        const std::string name = build_name(tmpl, first_number + i);
        FILE* f = fopen(name.c_str(), "wb");
        if (!f) { failed = 1; std::lock_guard<std::mutex> g(err_lock); if (first_error.empty()) first_error = "Error opening file '" + name + "'"; return; }
        const uint64_t len = off[i + 1] - off[i];
        if (len && fwrite(host + off[i], 1, len, f) != len) { failed = 1; std::lock_guard<std::mutex> g(err_lock); if (first_error.empty()) first_error = "short write to '" + name + "'"; }
        fclose(f);
        files++; bytes += len;
      }
    };
    uint32_t nt = threads ? threads : 8; if (nt > 64) nt = 64; if (nt > n) nt = (uint32_t)(n ? n : 1);
    std::vector<std::thread> ts;
    for (uint32_t t = 1; t < nt; t++) ts.emplace_back(work);
    work();
    for (auto& t : ts) t.join();
  }
  if (pinned) (void)hipHostFree(host); else free(host);
  if (files_written) *files_written = files.load();
  if (bytes_written) *bytes_written = bytes.load();
  if (not_written) *not_written = skipped.load();
  if (rc) return rc;
  if (failed.load()) { ctx->err = first_error; return EH_E_INVALID; }
  return EH_OK;
}
int eh_result_fetch(eh_ctx* ctx, uint64_t i, uint8_t* buf, uint64_t cap, uint64_t* out_len) {
  if (!ctx || !out_len) return EH_E_INVALID;
  int rc = result_ready(ctx); if (rc) return rc;
  if (i >= ctx->res.last_n) { ctx->err = "eh_result_fetch: case index outside the last batch"; return EH_E_INVALID; }
  uint64_t ol[2];
  HIPCHK(ctx, hipMemcpy(&ol[0], ctx->res.d_off + i, 8, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(&ol[1], ctx->res.d_len + i, 8, hipMemcpyDeviceToHost));
  *out_len = ol[1];
  if (ol[1] > cap || (!buf && ol[1])) { ctx->err = "eh_result_fetch: buffer too small"; return EH_E_INVALID; }
  if (ol[1]) HIPCHK(ctx, hipMemcpy(buf, ctx->res.d_out + ol[0], ol[1], hipMemcpyDeviceToHost));
  return EH_OK;
}
int eh_result_diag(eh_ctx* ctx, uint64_t* draws, int32_t* last_mutator) {
  if (!ctx) return EH_E_INVALID;
  int rc = result_ready(ctx); if (rc) return rc;
  uint64_t n = ctx->res.last_n;
  if (draws && n) HIPCHK(ctx, hipMemcpy(draws, ctx->res.d_draws, n * 8, hipMemcpyDeviceToHost));
  if (last_mutator && n) HIPCHK(ctx, hipMemcpy(last_mutator, ctx->res.d_lastm, n * 4, hipMemcpyDeviceToHost));
  return EH_OK;
}
int eh_result_cycles(eh_ctx* ctx, uint64_t* cycles) {
  if (!ctx || !cycles) return EH_E_INVALID;
  int rc = result_ready(ctx); if (rc) return rc;
  if (ctx->res.last_n) HIPCHK(ctx, hipMemcpy(cycles, ctx->res.d_cycles, ctx->res.last_n * 8, hipMemcpyDeviceToHost));
  return EH_OK;
}
int eh_result_meta(eh_ctx* ctx, uint64_t i, uint8_t* buf, uint64_t cap, uint64_t* n_events) {
  if (!ctx || !n_events) return EH_E_INVALID;
  int rc = result_ready(ctx, false); if (rc) return rc;
  if (!(ctx->flags & EH_FLAG_META_TRACE)) { ctx->err = "eh_result_meta: configure with EH_FLAG_META_TRACE"; return EH_E_STATE; }
  rc = eh_sync(ctx); if (rc) return rc;
  if (i >= ctx->res.last_n) { ctx->err = "eh_result_meta: case index outside the last batch"; return EH_E_INVALID; }
  uint64_t off = 0; uint32_t len = 0;
  HIPCHK(ctx, hipMemcpy(&off, ctx->res.d_toff + i, 8, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(&len, ctx->res.d_tlen + i, 4, hipMemcpyDeviceToHost));
  *n_events = len;                                                        // the trace's length whatever the buffer holds: (buf = NULL, cap = 0) asks for it
  const uint64_t take = buf ? (len < cap ? len : cap) : 0;                // "copied up to cap" (include/erlamsa_hip.h)
  // (with EH_FLAG_ORDERED_OUTPUT the traces stay in the completion-ordered arena, which is d_out2 after the swap)
  const uint8_t* src = (ctx->res.ordered ? ctx->res.d_out2 : ctx->res.d_out) + off;
  if (take) HIPCHK(ctx, hipMemcpy(buf, src, take, hipMemcpyDeviceToHost));
  return EH_OK;
}
int eh_result_peak(eh_ctx* ctx, uint64_t* peak) {
  if (!ctx || !peak) return EH_E_INVALID;
  int rc = result_ready(ctx); if (rc) return rc;
  if (ctx->res.last_n) HIPCHK(ctx, hipMemcpy(peak, ctx->res.d_peak, ctx->res.last_n * 8, hipMemcpyDeviceToHost));
  return EH_OK;
}
int eh_result_prof(eh_ctx* ctx, uint64_t* prof /* 256 values */) {
  if (!ctx || !prof) return EH_E_INVALID;
  int rc = result_ready(ctx); if (rc) return rc;
  HIPCHK(ctx, hipMemcpy(prof, ctx->res.d_counters.p->prof, sizeof(BatchCounters::prof), hipMemcpyDeviceToHost));
  return EH_OK;
}
