// eh_host_launch.h - host: a context's life, the device memory of a batch and its launch.
#pragma once
// Device memory of a mode-1 launch of up to n cases: the seeds and, behind them, the cases' profile ids; and the profile table.
const uint64_t SEED_ROW = 3 * sizeof(int64_t) + sizeof(uint32_t);
static int ensure_seeds(eh_ctx* ctx, uint64_t n) {
  HIPCHK(ctx, ctx->profiles.d_table.grow(MAX_PROFILES));
  HIPCHK(ctx, ctx->res.d_seeds.grow(n * SEED_ROW));
  return EH_OK;
}
static int64_t* seeds_of(eh_ctx* ctx) { return (int64_t*)ctx->res.d_seeds.p; }
static uint32_t* profile_ids_of(eh_ctx* ctx) { return (uint32_t*)(seeds_of(ctx) + 3 * (ctx->res.d_seeds.cap / SEED_ROW)); }

// (each array has a capacity of its own: any prefix of the growths may have succeeded when one fails)
static int ensure_results(eh_ctx* ctx, uint64_t n) {
  HIPCHK(ctx, ctx->res.d_cycles.grow(n));
  HIPCHK(ctx, ctx->res.d_peak.grow(n));
  HIPCHK(ctx, ctx->res.d_toff.grow(n));
  HIPCHK(ctx, ctx->res.d_tlen.grow(n));
  HIPCHK(ctx, ctx->res.d_off.grow(n));
  HIPCHK(ctx, ctx->res.d_len.grow(n));
  HIPCHK(ctx, ctx->res.d_status.grow(n));
  HIPCHK(ctx, ctx->res.d_draws.grow(n));
  HIPCHK(ctx, ctx->res.d_lastm.grow(n));
  return EH_OK;
}

// Device memory for batches of up to `n` cases over `in_bytes` input bytes: result arrays, the work-area pool, output
// arena.  Buffers only ever grow, so after eh_reserve (or a first batch of the largest size) no launch allocates or
// frees — hipFree synchronises the whole device.
static int reserve(eh_ctx* ctx, uint64_t n, uint64_t in_bytes) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_results(ctx, n ? n : 1);
  if (rc) return rc;
  uint64_t work_cap = ctx->max_case_bytes ? ctx->max_case_bytes : (8ull << 20);
  uint64_t big = ctx->big_case_bytes ? ctx->big_case_bytes : (32 * work_cap < (1024ull << 20) ? 32 * work_cap : (1024ull << 20));
  if (big < work_cap) big = work_cap;
  rc = pool_acquire(ctx, work_cap, big, ctx->pool_bytes_opt);
  if (rc) return rc;
  // a slot per workgroup of a batch: one workgroup per wavefront the device holds (EH_WAVES_PER_SIMD), or max_slots
  uint32_t want_slots = ctx->max_slots_opt ? ctx->max_slots_opt : (uint32_t)ctx->cus * 4u * EH_WAVES_PER_SIMD;
  if (want_slots > n) want_slots = (uint32_t)(n ? n : 1);
  uint64_t stride = (SLOT_TABLE_BYTES + work_cap + 255) & ~255ull;
  if (!ctx->d_slots || ctx->nslots < want_slots || ctx->slot_cap != work_cap) {
    HIPCHK(ctx, ctx->d_slots.reset(stride * want_slots));
    ctx->nslots = want_slots; ctx->slot_cap = work_cap; ctx->slot_stride = stride;
  }
  uint64_t want_out = ctx->out_capacity_opt ? ctx->out_capacity_opt : (8 * (in_bytes ? in_bytes : ctx->corpus.bytes) + (2048ull << 20));
  HIPCHK(ctx, ctx->res.d_out.grow(want_out));
  return EH_OK;
}

static int launch(eh_ctx* ctx, int mode, const int64_t seed[3], uint64_t first_case, uint64_t corpus_first, uint64_t n, hipStream_t st, bool profiled = false) {
  if (!ctx->configured || !ctx->corpus.d) { ctx->err = "configure and load a corpus first"; return EH_E_STATE; }
  if (corpus_first + n > ctx->corpus.n || (mode == 0 && first_case < 1)) { ctx->err = "case range outside the corpus"; return EH_E_INVALID; }
  // make_generator_fun (erlamsa_gen.erl:215-224) drops `file` without paths and `jump` with fewer than two: said aloud here
  if (ctx->corpus.n < (uint64_t)ctx->needs_paths || ctx->corpus.n > 0xFFFFFFFFull) { ctx->err = "generator file needs one corpus entry (path), jump two"; return EH_E_INVALID; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  uint64_t in_bytes = 0;
  if (!ctx->corpus.h_off.empty()) in_bytes = ctx->corpus.h_off[corpus_first + n] - ctx->corpus.h_off[corpus_first];
  int rc = reserve(ctx, n, in_bytes);
  if (rc) return rc;
  HIPCHK(ctx, ctx->res.d_counters.grow(1));
  HIPCHK(ctx, ctx->res.d_run.grow(1));
  HIPCHK(ctx, ctx->res.d_params.grow(1));
  if (!ctx->res.h_sum) { HIPCHK(ctx, hipHostMalloc((void**)&ctx->res.h_sum, sizeof(BatchSummary), hipHostMallocDefault)); memset(ctx->res.h_sum, 0, sizeof(BatchSummary)); }

  KParams p;
  memset(&p, 0, sizeof(p));
  p.corpus = dp(ctx->corpus.d); p.coff = dp(ctx->corpus.d_off); p.corpus_first = corpus_first; p.n_paths = ctx->corpus.n; p.n = n; p.first_case = first_case;
  p.mode = mode; p.run = dp(ctx->res.d_run); p.seeds = dp(seeds_of(ctx)); p.cfg = ctx->cfg;
  if (profiled) { p.profiles = dp(ctx->profiles.d_table); p.profile_id = dp(profile_ids_of(ctx)); }   // (memset above: nullptr otherwise)
  const DevPool* pl = ctx->pool;
  p.work_cap = pl->work_cap;
  p.work_budget = ctx->work_budget;                                            // 0 = no budget (the default)
  p.fuse_stream_min = ctx->fuse_stream_min;
  p.out = dp(ctx->res.d_out); p.out_cap = ctx->res.d_out.cap; p.out_cursor = dp(&ctx->res.d_counters.p->out_cursor);
  p.out_off = dp(ctx->res.d_off); p.out_len = dp(ctx->res.d_len); p.status = dp(ctx->res.d_status); p.draws = dp(ctx->res.d_draws); p.lastm = dp(ctx->res.d_lastm); p.cycles = dp(ctx->res.d_cycles); p.peak = dp(ctx->res.d_peak); p.trace_off = dp(ctx->res.d_toff); p.trace_len = dp(ctx->res.d_tlen); p.flags = ctx->flags;
  p.ctr = dp(ctx->res.d_counters); p.in_bytes = dp(&ctx->res.d_counters.p->in_bytes); p.prof = dp(ctx->res.d_counters.p->prof);
  p.slot_base = dp(ctx->d_slots); p.slot_stride = ctx->slot_stride;
  p.ntiers = pl->ntiers; p.pool_ctr = dp(pl->d_ctr); p.pool_cap[0] = pl->work_cap;
  p.board = (ctx->flags & EH_FLAG_NO_COOP) ? dp((CoBoard*)nullptr) : dp(pl->d_board);
  co_defaults(&p, ctx->cus);
  p.summary_out = dp(ctx->res.h_sum); p.batch_seq = ++ctx->res.batch_seq;
  if (n == 0) { memset(ctx->res.h_sum, 0, sizeof(BatchSummary)); ctx->res.h_sum->seq = ctx->res.batch_seq; }      // (no mutate kernel: nothing else would write it)
  for (int t = 1; t <= pl->ntiers; t++) { p.pool_base[t] = dp(pl->base[t]); p.pool_stride[t] = pl->stride[t]; p.pool_cap[t] = pl->cap[t]; p.pool_cnt[t] = pl->cnt[t]; p.pool_ring[t] = dp(pl->ring[t]); }
  // persistent workgroups, each pulling cases from the ticket counter.  Batches in flight on several streams may
  // oversubscribe the device: the dispatcher starts a batch's workgroups as those of earlier ones leave.
  uint32_t grid0 = ctx->nslots < n ? ctx->nslots : (uint32_t)n;

  // counters, argument block and run state by ONE one-wavefront kernel (no fill / copy kernels of the runtime: see eh_prologue_kernel)
  hipLaunchKernelGGL(eh_prologue_kernel, dim3(1), dim3(64), 0, st, p, mode == 0 ? seed[0] : 0, mode == 0 ? seed[1] : 0, mode == 0 ? seed[2] : 0,
                     ctx->res.d_run, ctx->res.d_params, (unsigned long long*)ctx->res.d_counters.p);
  HIPCHK(ctx, hipEventRecord(ctx->res.ev0, st));
  if (n > 0) hipLaunchKernelGGL(eh_mutate_kernel, dim3(grid0), dim3(64), 0, st, (const KParams*)ctx->res.d_params);
  HIPCHK(ctx, hipEventRecord(ctx->res.ev1, st));
  HIPCHK(ctx, hipGetLastError());
  ctx->res.ordered = false;
  if ((ctx->flags & EH_FLAG_ORDERED_OUTPUT) && n > 0) {
    // second arena + ordered offsets, then scan + gather on the same stream; the arenas swap roles so that
    // eh_result_device / eh_result_download see one contiguous case-ordered buffer
    HIPCHK(ctx, ctx->res.d_out2.grow(ctx->res.d_out.cap));
    HIPCHK(ctx, ctx->res.d_ord.grow(n + 1));
    hipLaunchKernelGGL(eh_order_scan_kernel, dim3(1), dim3(64), 0, st, ctx->res.d_len, ctx->res.d_ord, n);
    uint32_t g = (uint32_t)ctx->cus * 32u; if (g > n) g = (uint32_t)n;
    hipLaunchKernelGGL(eh_order_gather_kernel, dim3(g), dim3(64), 0, st, ctx->res.d_out, ctx->res.d_out2, ctx->res.d_off, ctx->res.d_len, ctx->res.d_ord, n, 0ull);
    HIPCHK(ctx, hipMemcpyAsync(ctx->res.d_off, ctx->res.d_ord, n * 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipGetLastError());
    ctx->res.d_out.swap(ctx->res.d_out2);
    ctx->res.ordered = true;
  }
  ctx->res.last_stream = st; ctx->res.last_n = n; ctx->res.last_in_bytes = in_bytes; ctx->res.have_result = true;
  return EH_OK;
}

int eh_create(int device, eh_ctx** out) {
  if (!out) return EH_E_INVALID;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return EH_E_NODEVICE;
  eh_ctx* ctx = new (std::nothrow) eh_ctx();
  if (!ctx) return EH_E_NOMEM;
  ctx->device = device;
  if (hipSetDevice(device) != hipSuccess) { delete ctx; return EH_E_NODEVICE; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) { delete ctx; return EH_E_NODEVICE; }
  ctx->cus = prop.multiProcessorCount;
  // (Until round 5 the kernel recursed - nested scheduler calls of b64 / sgm / js - and eh_create raised hipLimitStackSize to 6 KiB per lane
  // for the whole process.  The scheduler is a loop over explicit frames now (eh_device.h mux_fuzzers): the kernel's stack is the 1.8 KiB
  // the assembler adds up, and no limit of the process is touched.)
  // (the constant tables - AS183 powers, CRC-32, funny_unicode/0 - are initialised in the code object: eh_device.h, eh_zlib.h)
  if (hipEventCreate(&ctx->res.ev0) != hipSuccess || hipEventCreate(&ctx->res.ev1) != hipSuccess) {
    eh_destroy(ctx);
    return EH_E_HIP;
  }
  *out = ctx;
  return EH_OK;
}

void eh_destroy(eh_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  if (ctx->comm) { ehcomm::Api* a = ehcomm::api(); if (a->h) (void)a->CommDestroy(ctx->comm); ctx->comm = nullptr; }
  pool_release(ctx);
  delete ctx;                                          // (buffers and handles go with the parts that own them: after the synchronise above)
}

int eh_reserve(eh_ctx* ctx, uint64_t max_cases) {
  if (!ctx) return EH_E_INVALID;
  if (!ctx->configured || !ctx->corpus.d) { ctx->err = "configure and load a corpus first"; return EH_E_STATE; }
  std::lock_guard<std::mutex> g(ctx->co_lock);
  int rc = reserve(ctx, max_cases, 0);
  return rc ? rc : ensure_seeds(ctx, max_cases);     // (per-call seeds and profile ids: eh_fuzz_calls / eh_fuzz_calls_profiled never allocate either)
}

int eh_fuzz_batch(eh_ctx* ctx, const int64_t seed[3], uint64_t first_case, uint64_t corpus_first, uint64_t n, void* stream) {
  if (!ctx || !seed) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  return launch(ctx, 0, seed, first_case, corpus_first, n, (hipStream_t)stream);
}
// co_lock held (fuzz_calls_idle, co_launch): per-case seeds, and profile ids where `profile` is not NULL
static int fuzz_calls(eh_ctx* ctx, const int64_t* seeds, const uint32_t* profile, uint64_t corpus_first, uint64_t n, void* stream) {
  if (profile) {
    if (!ctx->configured) { ctx->err = "configure first"; return EH_E_STATE; }
    const uint32_t count = (uint32_t)ctx->profiles.list.size();
    for (uint64_t i = 0; i < n; i++) if (profile[i] >= count) { ctx->err = "case " + std::to_string(i) + ": no profile " + std::to_string(profile[i]) + " (eh_profile_count = " + std::to_string(count) + ")"; return EH_E_INVALID; }
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_seeds(ctx, n);
  if (rc) return rc;
  // synchronous copies: the caller's arrays may be freed or reused as soon as this call returns
  if (n) { HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream)); HIPCHK(ctx, hipMemcpy(seeds_of(ctx), seeds, n * 24, hipMemcpyHostToDevice)); }
  if (profile && n) {
    HIPCHK(ctx, hipMemcpy(profile_ids_of(ctx), profile, n * 4, hipMemcpyHostToDevice));
    // profiles added since the last profiled launch.  The context's previous batch on this stream has ended (the wait above), and
    // entries below profiles_on_device are never rewritten: no kernel reads what is copied here.
    const uint32_t have = ctx->profiles.on_device, count = (uint32_t)ctx->profiles.list.size();
    if (count > have) HIPCHK(ctx, hipMemcpy(ctx->profiles.d_table + have, ctx->profiles.list.data() + have, (size_t)(count - have) * sizeof(ProfileCfg), hipMemcpyHostToDevice));
    ctx->profiles.on_device = count;
  }
  int64_t dummy[3] = {0, 0, 0};
  return launch(ctx, 1, dummy, 1, corpus_first, n, (hipStream_t)stream, profile != nullptr && n > 0);
}
static int fuzz_calls_idle(eh_ctx* ctx, const int64_t* seeds, const uint32_t* profile, uint64_t corpus_first, uint64_t n, void* stream) {
  if (!ctx || !seeds) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock); if (int rc = co_idle(ctx)) return rc;
  return fuzz_calls(ctx, seeds, profile, corpus_first, n, stream);
}
int eh_fuzz_calls(eh_ctx* ctx, const int64_t* seeds, uint64_t corpus_first, uint64_t n, void* stream) {
  return fuzz_calls_idle(ctx, seeds, nullptr, corpus_first, n, stream);
}
int eh_fuzz_calls_profiled(eh_ctx* ctx, const int64_t* seeds, const uint32_t* profile, uint64_t corpus_first, uint64_t n, void* stream) {
  if (!profile) return EH_E_INVALID;
  return fuzz_calls_idle(ctx, seeds, profile, corpus_first, n, stream);
}

int eh_sync(eh_ctx* ctx) {
  if (!ctx) return EH_E_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->res.last_stream));
  return EH_OK;
}

int eh_stream(eh_ctx* ctx, void** stream) {
  if (!ctx || !stream) return EH_E_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // (streams of different priorities - high / normal / low in turn over the contexts - were measured against the convoy of passes
  // launched together: 84.6 against 84.9 GB/s, profiles/r06_stream_priorities_and_slots.txt; not kept)
  if (!ctx->res.own_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->res.own_stream, hipStreamNonBlocking));
  *stream = (void*)ctx->res.own_stream;
  return EH_OK;
}

int eh_host_alloc(void** p, uint64_t bytes) {
  if (!p) return EH_E_INVALID;
  *p = nullptr;
  return hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? EH_OK : EH_E_NOMEM;
}
void eh_host_free(void* p) { if (p) (void)hipHostFree(p); }

// Has the last batch of this context finished (results ready, the context free for the next batch)?  Never blocks: what a host
// that keeps several contexts busy polls to give the next batch to WHICHEVER context is free, instead of waiting for the oldest.
int eh_batch_done(eh_ctx* ctx, int* done) {
  if (!ctx || !done) return EH_E_INVALID;
  *done = 1;
  if (!ctx->res.have_result) return EH_OK;
  hipError_t e = hipEventQuery(ctx->res.ev1);
  if (e == hipSuccess) return EH_OK;
  if (e == hipErrorNotReady) { *done = 0; (void)hipGetLastError(); return EH_OK; }
  ctx->err = std::string("hipEventQuery: ") + hipGetErrorString(e);
  return EH_E_HIP;
}
int eh_last_kernel_ms(eh_ctx* ctx, float* ms) {
  if (!ctx || !ms) return EH_E_INVALID;
  if (int rc = result_ready(ctx, false)) return rc;
  HIPCHK(ctx, hipEventSynchronize(ctx->res.ev1));
  HIPCHK(ctx, hipEventElapsedTime(ms, ctx->res.ev0, ctx->res.ev1));
  return EH_OK;
}
