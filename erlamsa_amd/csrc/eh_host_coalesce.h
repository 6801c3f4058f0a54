// eh_host_coalesce.h - host: request coalescing (eh_submit / eh_flush / eh_poll) over the bookkeeping of eh_coalesce.h.
#pragma once
// Brings the launched batch's results to the host (one download) and files them under their tickets.
// `lk` is the caller's hold on co_lock: the wait for the batch and the download happen WITHOUT it, so that other threads keep
// submitting to the next batch meanwhile; a second collector waits for the first.
static int co_collect(eh_ctx* ctx, std::unique_lock<std::mutex>& lk) {
  ctx->co_cv.wait(lk, [ctx] { return !ctx->co_collecting; });
  if (!ctx->co.in_flight) return EH_OK;
  ctx->co_collecting = true;
  const std::vector<uint64_t> tickets = ctx->co.flying;
  const uint64_t n = tickets.size();
  lk.unlock();
  uint64_t in_b = 0, out_b = 0, nc = 0;
  std::vector<uint8_t> data; std::vector<uint64_t> off(n + 1); std::vector<int32_t> st(n ? n : 1);
  int rc = result_totals(ctx, &in_b, &out_b, &nc);
  if (!rc && nc != n) { ctx->err = "coalescer: the context's last batch is not the one that was flushed"; rc = EH_E_STATE; }
  if (!rc) { data.resize(out_b ? out_b : 1); rc = result_download(ctx, data.data(), data.size(), off.data(), st.data()); }
  lk.lock();
  if (!rc) ctx->co.collected(tickets, data.data(), off.data(), st.data());   // (a failed download: the batch stays in flight)
  ctx->co_collecting = false; ctx->co_cv.notify_all();
  return rc;
}
// Launches the pending batch (after collecting the previous one: one result buffer per context).
static int co_launch(eh_ctx* ctx, std::unique_lock<std::mutex>& lk) {
  if (!ctx->co.pending.size()) return EH_OK;
  int rc = co_collect(ctx, lk);
  if (rc) return rc;
  const CoBatch& b = ctx->co.pending;
  if (!b.size()) return EH_OK;                                      // (co_collect lets other threads in: one of them has launched the batch)
  rc = corpus_upload(ctx, b.data.data(), b.off.data(), b.size());
  // requests that all run under profile 0 take the unprofiled launch
  if (!rc) rc = fuzz_calls(ctx, b.seeds.data(), b.profiled() ? b.profile.data() : nullptr, 0, b.size(), nullptr);
  if (!rc) ctx->co.launched();
  return rc;
}
int eh_coalesce_limits(eh_ctx* ctx, uint64_t flush_cases, uint64_t flush_bytes) {
  if (!ctx || !flush_cases || !flush_bytes) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock);
  ctx->co.flush_cases = flush_cases; ctx->co.flush_bytes = flush_bytes;
  return EH_OK;
}
int eh_submit(eh_ctx* ctx, const uint8_t* data, uint64_t len, const int64_t seed[3], uint64_t* ticket) {
  return eh_submit_profiled(ctx, data, len, seed, 0, ticket);
}
int eh_submit_profiled(eh_ctx* ctx, const uint8_t* data, uint64_t len, const int64_t seed[3], uint32_t profile, uint64_t* ticket) {
  if (!ctx || !seed || !ticket || (!data && len)) return EH_E_INVALID;
  if (!ctx->configured) { ctx->err = "configure first"; return EH_E_STATE; }
  std::unique_lock<std::mutex> lk(ctx->co_lock);
  if (profile >= ctx->profiles.list.size()) { ctx->err = "no profile " + std::to_string(profile) + " (eh_profile_count = " + std::to_string(ctx->profiles.list.size()) + ")"; return EH_E_INVALID; }
  const uint64_t mine = ctx->co.next_ticket;
  if (!ctx->co.pending.push(mine, data, len, seed, profile)) return EH_E_NOMEM;
  ctx->co.next_ticket++;                                  // (before any launch: co_collect lets other submitters in)
  if (ctx->co.at_limit()) {
    int rc = co_launch(ctx, lk);
    // a launch that fails takes this request back out (the caller gets no ticket for it); the others stay queued for the next flush
    if (rc) { (void)ctx->co.cancel(mine); return rc; }
  }
  *ticket = mine;
  return EH_OK;
}
int eh_cancel(eh_ctx* ctx, uint64_t ticket) {
  if (!ctx) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock);
  int rc = ctx->co.cancel(ticket);
  if (rc) ctx->err = "unknown or already consumed ticket";
  return rc;
}
int eh_flush(eh_ctx* ctx) {
  if (!ctx) return EH_E_INVALID;
  std::unique_lock<std::mutex> lk(ctx->co_lock);
  return co_launch(ctx, lk);
}
int eh_poll(eh_ctx* ctx, uint64_t ticket, uint8_t* out, uint64_t cap, uint64_t* out_len, int32_t* status) {
  if (!ctx || !out_len || !status) return EH_E_INVALID;
  std::unique_lock<std::mutex> lk(ctx->co_lock);
  const CoWhere w = ctx->co.where(ticket);
  if (w == CoWhere::pending) return EH_E_AGAIN;
  if (w == CoWhere::unknown) { ctx->err = "unknown or already consumed ticket"; return EH_E_INVALID; }
  if (w == CoWhere::in_flight) { int rc = co_collect(ctx, lk); if (rc) return rc; }   // waits for the batch
  auto it = ctx->co.done.find(ticket);
  *out_len = it->second.out.size(); *status = it->second.status;
  if (it->second.out.size() > cap || (!out && !it->second.out.empty())) { ctx->err = "eh_poll: buffer too small"; return EH_E_INVALID; }
  if (!it->second.out.empty()) memcpy(out, it->second.out.data(), it->second.out.size());
  ctx->co.done.erase(it);
  return EH_OK;
}
