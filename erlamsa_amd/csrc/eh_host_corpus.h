// eh_host_corpus.h - host: the corpus of a context - uploaded, attached, or spread over several GPUs with RCCL (eh_comm.h).
#pragma once
// The corpus becomes the filled buffers (d, doff); what the context owned before goes with them when the caller returns.
static void adopt_corpus(eh_ctx* ctx, DevBuf<uint8_t>& d, DevBuf<uint64_t>& doff, uint64_t n, uint64_t nbytes) {
  ctx->corpus.own.swap(d); ctx->corpus.own_off.swap(doff);
  ctx->corpus.d = ctx->corpus.own; ctx->corpus.d_off = ctx->corpus.own_off; ctx->corpus.n = n; ctx->corpus.bytes = nbytes;
}
static int corpus_upload(eh_ctx* ctx, const uint8_t* data, const uint64_t* off, uint64_t n) {   // co_lock held (eh_corpus_upload, co_launch)
  HIPCHK(ctx, hipSetDevice(ctx->device));
  uint64_t nbytes = off[n];
  HIPCHK(ctx, hipDeviceSynchronize());                       // no launch may still read the previous corpus
  if (ctx->corpus.own.cap >= nbytes && ctx->corpus.own_off.cap >= n + 1) {      // steady state of a service: no hipMalloc / hipFree (an attached corpus: nothing is owned)
    if (nbytes) HIPCHK(ctx, hipMemcpy(ctx->corpus.d, data, nbytes, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->corpus.d_off, off, (n + 1) * 8, hipMemcpyHostToDevice));
    ctx->corpus.h_off.assign(off, off + n + 1);
    ctx->corpus.n = n; ctx->corpus.bytes = nbytes;
    return EH_OK;
  }
  DevBuf<uint8_t> d; DevBuf<uint64_t> doff;                  // (the corpus in use stays until the new one is complete)
  hipError_t e = d.grow(nbytes + nbytes / 2 + 4096);         // room to grow
  if (e == hipSuccess) e = doff.grow(n + n / 2 + 16);
  if (e == hipSuccess && nbytes) e = hipMemcpy(d, data, nbytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(doff, off, (n + 1) * 8, hipMemcpyHostToDevice);
  HIPCHK(ctx, e);
  ctx->corpus.h_off.assign(off, off + n + 1);
  adopt_corpus(ctx, d, doff, n, nbytes);
  return EH_OK;
}
int eh_corpus_upload(eh_ctx* ctx, const uint8_t* data, const uint64_t* off, uint64_t n) {
  if (!ctx || !off || (!data && off[n] > 0)) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  return corpus_upload(ctx, data, off, n);
}
int eh_corpus_attach(eh_ctx* ctx, const void* d_data, const void* d_off, uint64_t n, uint64_t nbytes) {
  if (!ctx || !d_off) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ctx->corpus.h_off.resize(n + 1);
  HIPCHK(ctx, hipMemcpy(ctx->corpus.h_off.data(), d_off, (n + 1) * 8, hipMemcpyDeviceToHost));
  if (ctx->corpus.h_off[n] != nbytes) { ctx->err = "off[n] != nbytes"; return EH_E_INVALID; }
  ctx->corpus.own.release(); ctx->corpus.own_off.release();
  ctx->corpus.d = (uint8_t*)d_data; ctx->corpus.d_off = (uint64_t*)d_off; ctx->corpus.n = n; ctx->corpus.bytes = nbytes;
  return EH_OK;
}

int eh_corpus_device(eh_ctx* ctx, const void** d_data, const void** d_off, uint64_t* n, uint64_t* nbytes) {
  if (!ctx) return EH_E_INVALID;
  if (!ctx->corpus.d) { ctx->err = "no corpus loaded"; return EH_E_STATE; }
  if (d_data) *d_data = ctx->corpus.d;
  if (d_off) *d_off = ctx->corpus.d_off;
  if (n) *n = ctx->corpus.n;
  if (nbytes) *nbytes = ctx->corpus.bytes;
  return EH_OK;
}

// ---- multi-GPU: the arena over RCCL (eh_comm.h) ------------------------------------------------------------------------------
#define NCCLCHK(ctx, a, call)                                                                                   \
  do {                                                                                                          \
    int r_ = (call);                                                                                            \
    if (r_ != 0) { (ctx)->err = std::string(#call) + ": " + ((a)->GetErrorString ? (a)->GetErrorString(r_) : "RCCL error"); return EH_E_HIP; } \
  } while (0)

// an owned corpus buffer for n entries / nbytes bytes (contents undefined); keeps the one it has when that is large enough
static int corpus_own_buffers(eh_ctx* ctx, uint64_t n, uint64_t nbytes) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipDeviceSynchronize());                       // no launch may still read the previous corpus
  if (ctx->corpus.own.cap >= nbytes && ctx->corpus.own_off.cap >= n + 1) { ctx->corpus.n = n; ctx->corpus.bytes = nbytes; return EH_OK; }
  DevBuf<uint8_t> d; DevBuf<uint64_t> doff;
  hipError_t e = d.grow(nbytes + 4096);
  if (e == hipSuccess) e = doff.grow(n + 16);
  HIPCHK(ctx, e);
  adopt_corpus(ctx, d, doff, n, nbytes);
  return EH_OK;
}

int eh_device_count(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess && n > 0 ? n : 0; }
int eh_comm_unique_id(uint8_t id[128]) {
  if (!id) return EH_E_INVALID;
  ehcomm::Api* a = ehcomm::api();
  if (!a->h) return EH_E_UNSUPPORTED;
  ehcomm::UniqueId u;
  if (a->GetUniqueId(&u) != 0) return EH_E_HIP;
  memcpy(id, u.internal, 128);
  return EH_OK;
}
int eh_comm_init(eh_ctx* ctx, const uint8_t id[128], int rank, int nranks) {
  if (!ctx || !id || nranks < 1 || rank < 0 || rank >= nranks) return EH_E_INVALID;
  ehcomm::Api* a = ehcomm::api();
  if (!a->h) { ctx->err = a->err; return EH_E_UNSUPPORTED; }
  if (ctx->comm) { (void)a->CommDestroy(ctx->comm); ctx->comm = nullptr; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ehcomm::UniqueId u; memcpy(u.internal, id, 128);
  NCCLCHK(ctx, a, a->CommInitRank(&ctx->comm, nranks, u, rank));
  ctx->comm_rank = rank; ctx->comm_n = nranks;
  return EH_OK;
}
int eh_comm_init_local(eh_ctx** ctxs, int nctx) {
  if (!ctxs || nctx < 1 || nctx > 64) return EH_E_INVALID;
  for (int i = 0; i < nctx; i++) if (!ctxs[i]) return EH_E_INVALID;
  ehcomm::Api* a = ehcomm::api();
  if (!a->h) { ctxs[0]->err = a->err; return EH_E_UNSUPPORTED; }
  std::vector<int> devs(nctx); std::vector<ehcomm::Comm> comms(nctx, nullptr);
  for (int i = 0; i < nctx; i++) {
    devs[i] = ctxs[i]->device;
    for (int j = 0; j < i; j++) if (devs[j] == devs[i]) { ctxs[0]->err = "eh_comm_init_local: one context per device (contexts of one device share the corpus with eh_corpus_device / eh_corpus_attach)"; return EH_E_INVALID; }
    if (ctxs[i]->comm) { (void)a->CommDestroy(ctxs[i]->comm); ctxs[i]->comm = nullptr; }
  }
  NCCLCHK(ctxs[0], a, a->CommInitAll(comms.data(), nctx, devs.data()));
  for (int i = 0; i < nctx; i++) { ctxs[i]->comm = comms[i]; ctxs[i]->comm_rank = i; ctxs[i]->comm_n = nctx; }
  return EH_OK;
}
int eh_comm_destroy(eh_ctx* ctx) {
  if (!ctx) return EH_E_INVALID;
  if (ctx->comm) { ehcomm::Api* a = ehcomm::api(); if (a->h) (void)a->CommDestroy(ctx->comm); ctx->comm = nullptr; }
  ctx->comm_rank = 0; ctx->comm_n = 1;
  return EH_OK;
}

// One process per GPU.  Root hands over the arena (host pointers), the others pass NULL / 0; afterwards every rank's context holds
// the corpus as after eh_corpus_upload.  Three collectives on the context's stream: the sizes, the bytes, the offsets.
int eh_corpus_broadcast(eh_ctx* ctx, int root, const uint8_t* data, const uint64_t* off, uint64_t n) {
  if (!ctx) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  if (!ctx->comm) { ctx->err = "eh_comm_init first"; return EH_E_STATE; }
  if (root < 0 || root >= ctx->comm_n) return EH_E_INVALID;
  const bool is_root = ctx->comm_rank == root;
  if (is_root && (!off || (!data && off[n] > 0))) return EH_E_INVALID;
  ehcomm::Api* a = ehcomm::api();
  HIPCHK(ctx, hipSetDevice(ctx->device));
  void* stv = nullptr; int rc = eh_stream(ctx, &stv); if (rc) return rc;
  hipStream_t st = (hipStream_t)stv;
  DevBuf<uint64_t> d_hdr;
  HIPCHK(ctx, d_hdr.grow(2));
  uint64_t hdr[2] = {is_root ? n : 0, is_root ? off[n] : 0};
  if (is_root) HIPCHK(ctx, hipMemcpy(d_hdr, hdr, 16, hipMemcpyHostToDevice));
  NCCLCHK(ctx, a, a->Broadcast(d_hdr, d_hdr, 2, ehcomm::kUint64, root, ctx->comm, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  HIPCHK(ctx, hipMemcpy(hdr, d_hdr, 16, hipMemcpyDeviceToHost));
  const uint64_t cn = hdr[0], nbytes = hdr[1];
  // (A rank that fails locally between the header and the payload - out of memory here - leaves its peers in the next collective:
  // there is no way to call them back.  The caller's answer to an error from this function is eh_comm_destroy on every rank,
  // ncclCommAbort's effect on the peers, and a fresh communicator; include/erlamsa_hip.h says so.)
  rc = corpus_own_buffers(ctx, cn, nbytes); if (rc) return rc;
  if (is_root) {
    if (nbytes) HIPCHK(ctx, hipMemcpy(ctx->corpus.d, data, nbytes, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->corpus.d_off, off, (cn + 1) * 8, hipMemcpyHostToDevice));
  }
  if (nbytes) NCCLCHK(ctx, a, a->Broadcast(ctx->corpus.d, ctx->corpus.d, nbytes, ehcomm::kUint8, root, ctx->comm, st));
  NCCLCHK(ctx, a, a->Broadcast(ctx->corpus.d_off, ctx->corpus.d_off, cn + 1, ehcomm::kUint64, root, ctx->comm, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  ctx->corpus.h_off.resize(cn + 1);
  if (is_root) ctx->corpus.h_off.assign(off, off + cn + 1);
  else HIPCHK(ctx, hipMemcpy(ctx->corpus.h_off.data(), ctx->corpus.d_off, (cn + 1) * 8, hipMemcpyDeviceToHost));
  if (ctx->corpus.h_off[cn] != nbytes) { ctx->err = "eh_corpus_broadcast: the offsets that arrived do not end at the arena's size"; return EH_E_HIP; }
  return EH_OK;
}

// Every rank gives ITS shard - the same number of entries and of bytes on every rank (BASELINE configs[4]: fixed-size seeds) -;
// afterwards every context holds the shards in rank order as one corpus.  In place: the shard is uploaded where it belongs and
// ncclAllGather fills in the others, so each xGMI link carries 1/nranks of the arena.
int eh_corpus_allgather(eh_ctx* ctx, const uint8_t* data, const uint64_t* off, uint64_t n_local) {
  if (!ctx || !off || (!data && off[n_local] > 0)) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  if (!ctx->comm) { ctx->err = "eh_comm_init first"; return EH_E_STATE; }
  ehcomm::Api* a = ehcomm::api();
  HIPCHK(ctx, hipSetDevice(ctx->device));
  void* stv = nullptr; int rc = eh_stream(ctx, &stv); if (rc) return rc;
  hipStream_t st = (hipStream_t)stv;
  const int R = ctx->comm_n, me = ctx->comm_rank;
  const uint64_t B = off[n_local];
  // do all ranks bring the same shape?
  DevBuf<uint64_t> d_sz;
  HIPCHK(ctx, d_sz.grow(2 * (uint64_t)R));
  uint64_t mine[2] = {n_local, B};
  HIPCHK(ctx, hipMemcpy(d_sz + 2 * me, mine, 16, hipMemcpyHostToDevice));
  NCCLCHK(ctx, a, a->AllGather(d_sz + 2 * me, d_sz, 2, ehcomm::kUint64, ctx->comm, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  std::vector<uint64_t> sz(2 * (size_t)R);
  HIPCHK(ctx, hipMemcpy(sz.data(), d_sz, 16 * (size_t)R, hipMemcpyDeviceToHost));
  for (int r = 0; r < R; r++) if (sz[2 * r] != n_local || sz[2 * r + 1] != B) { ctx->err = "eh_corpus_allgather: shards differ in entries or bytes between ranks (use eh_corpus_broadcast)"; return EH_E_INVALID; }
  const uint64_t cn = n_local * (uint64_t)R, nbytes = B * (uint64_t)R;
  rc = corpus_own_buffers(ctx, cn, nbytes); if (rc) return rc;
  if (B) HIPCHK(ctx, hipMemcpy(ctx->corpus.d + B * me, data, B, hipMemcpyHostToDevice));
  std::vector<uint64_t> lo(n_local ? n_local : 1);
  for (uint64_t i = 0; i < n_local; i++) lo[i] = off[i] + B * me;
  if (n_local) HIPCHK(ctx, hipMemcpy(ctx->corpus.d_off + n_local * me, lo.data(), n_local * 8, hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(ctx->corpus.d_off + cn, &nbytes, 8, hipMemcpyHostToDevice));
  if (B) NCCLCHK(ctx, a, a->AllGather(ctx->corpus.d + B * me, ctx->corpus.d, B, ehcomm::kUint8, ctx->comm, st));
  if (n_local) NCCLCHK(ctx, a, a->AllGather(ctx->corpus.d_off + n_local * me, ctx->corpus.d_off, n_local, ehcomm::kUint64, ctx->comm, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  ctx->corpus.h_off.resize(cn + 1);
  HIPCHK(ctx, hipMemcpy(ctx->corpus.h_off.data(), ctx->corpus.d_off, (cn + 1) * 8, hipMemcpyDeviceToHost));
  return EH_OK;
}

// One process, several GPUs (a BEAM node): the corpus loaded on ctxs[root] goes to the devices of all the others (grouped
// ncclBroadcast over the communicators of eh_comm_init_local).
int eh_corpus_broadcast_local(eh_ctx** ctxs, int nctx, int root) {
  if (!ctxs || nctx < 1 || root < 0 || root >= nctx) return EH_E_INVALID;
  for (int i = 0; i < nctx; i++) if (!ctxs[i] || !ctxs[i]->comm || ctxs[i]->comm_n != nctx || ctxs[i]->comm_rank != i) { if (ctxs[0]) ctxs[0]->err = "eh_comm_init_local on these contexts, in this order, first"; return EH_E_STATE; }
  eh_ctx* r = ctxs[root];
  if (!r->corpus.d) { r->err = "no corpus loaded on the root context"; return EH_E_STATE; }
  ehcomm::Api* a = ehcomm::api();
  const uint64_t cn = r->corpus.n, nbytes = r->corpus.bytes;
  std::vector<hipStream_t> sts(nctx);
  for (int i = 0; i < nctx; i++) {
    eh_ctx* x = ctxs[i];
    if (i != root) { int rc = corpus_own_buffers(x, cn, nbytes); if (rc) return rc; }
    void* stv = nullptr; int rc = eh_stream(x, &stv); if (rc) return rc;
    sts[i] = (hipStream_t)stv;
  }
  NCCLCHK(r, a, a->GroupStart());
  // (whatever fails inside the group, the group is ENDED before the function returns: an open group swallows every later call)
  int grc = EH_OK; eh_ctx* gbad = r; std::string gerr;
  for (int i = 0; i < nctx && grc == EH_OK; i++) {
    eh_ctx* x = ctxs[i];
    hipError_t he = hipSetDevice(x->device);
    if (he != hipSuccess) { grc = EH_E_HIP; gbad = x; gerr = std::string("hipSetDevice: ") + hipGetErrorString(he); break; }
    int nr = nbytes ? a->Broadcast(x->corpus.d, x->corpus.d, nbytes, ehcomm::kUint8, root, x->comm, sts[i]) : 0;
    if (nr == 0) nr = a->Broadcast(x->corpus.d_off, x->corpus.d_off, cn + 1, ehcomm::kUint64, root, x->comm, sts[i]);
    if (nr != 0) { grc = EH_E_HIP; gbad = x; gerr = std::string("ncclBroadcast: ") + (a->GetErrorString ? a->GetErrorString(nr) : "RCCL error"); }
  }
  const int ge = a->GroupEnd();
  if (grc != EH_OK) { gbad->err = gerr; if (gbad != ctxs[0]) ctxs[0]->err = gerr; return grc; }
  if (ge != 0) { r->err = std::string("ncclGroupEnd: ") + (a->GetErrorString ? a->GetErrorString(ge) : "RCCL error"); return EH_E_HIP; }
  for (int i = 0; i < nctx; i++) {
    eh_ctx* x = ctxs[i];
    HIPCHK(x, hipSetDevice(x->device));
    HIPCHK(x, hipStreamSynchronize(sts[i]));
    if (i != root) x->corpus.h_off = r->corpus.h_off;
  }
  return EH_OK;
}
