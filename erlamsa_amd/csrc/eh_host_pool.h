// eh_host_pool.h - host: the work-area pool that the contexts of a device share, and the cooperative-execution thresholds.
#pragma once
// ---- the work-area pool ------------------------------------------------------------------------------------------
// One pool per (device, max_case_bytes, big_case_bytes, pool_bytes), shared by all contexts that ask for those sizes and
// freed with the last of them.  Tier 0 has one slot (block tables + max_case_bytes) for every wavefront the device can hold
// of eh_mutate_kernel — workgroups of any number of batches in flight, on any streams, take their slot from it — and
// tiers 1.. hold the larger areas (4x per tier up to big_case_bytes) a wavefront borrows for a case that outgrew its slot.
static std::mutex g_pool_lock;
static std::vector<DevPool*> g_pools;

static void pool_free(DevPool* pl) {
  (void)hipSetDevice(pl->device);
  (void)hipDeviceSynchronize();
  delete pl;
}
static void pool_release(eh_ctx* ctx) {
  if (!ctx->pool) return;
  std::lock_guard<std::mutex> g(g_pool_lock);
  DevPool* pl = ctx->pool; ctx->pool = nullptr;
  if (--pl->refs > 0) return;
  for (size_t i = 0; i < g_pools.size(); i++) if (g_pools[i] == pl) { g_pools.erase(g_pools.begin() + i); break; }
  pool_free(pl);
}
static int pool_acquire(eh_ctx* ctx, uint64_t work_cap, uint64_t big, uint64_t pool_bytes_opt) {
  if (ctx->pool && ctx->pool->work_cap == work_cap && ctx->pool->big == big && ctx->pool->pool_bytes_opt == pool_bytes_opt) return EH_OK;
  pool_release(ctx);
  std::lock_guard<std::mutex> g(g_pool_lock);
  for (DevPool* q : g_pools)
    if (q->device == ctx->device && q->work_cap == work_cap && q->big == big && q->pool_bytes_opt == pool_bytes_opt) { q->refs++; ctx->pool = q; return EH_OK; }
  DevPool* pl = new (std::nothrow) DevPool();
  if (!pl) return EH_E_NOMEM;
  pl->device = ctx->device; pl->work_cap = work_cap; pl->big = big; pl->pool_bytes_opt = pool_bytes_opt;
  pl->cap[0] = work_cap;
  // twice the area per tier (most cases that outgrow what they hold need less than twice as much); the last tier has `big`.
  // The pool's memory (pool_bytes; default: a quarter of the free memory, at most 64 GiB) is split over the tiers in the
  // proportions the bench workload asks for them (BASELINE configs[2], 4 MiB slots: by far most borrowers are fuse calls on
  // blocks of 0.1-1 MB, whose tables take 5-20 MB): 12 / 23 / 17 / 7 / 10 / 10 / 9 / 12 percent from the smallest tier up.
  // Every tier holds at least one area, at most 4096; a tier that cannot be allocated at all ends the ladder.
  // Round 4: the large tiers get three times what they had.  With 2 areas of 1 GiB and 2 of 512 MiB for six passes in flight the
  // heaviest cases of the passes queued for each other (eh_pool_stats of a bench run: ~130 waits of 1.8 G ticks each for the last
  // tier alone, 1.8 - 3.2 T ticks of sleeping wavefronts per run), which stretched exactly the cases that decide how long a pass lasts.
  uint32_t SHARE[POOL_TIERS] = {12, 23, 17, 7, 10, 10, 9, 12};
  if (const char* ev = getenv("EH_POOL_SHARES")) {                                 // (measurement knob: eight numbers, smallest tier first)
    uint32_t v[POOL_TIERS]; int k = 0;
    for (const char* q = ev; *q && k < POOL_TIERS; ) { char* end = nullptr; unsigned long x = strtoul(q, &end, 10); if (end == q) break; v[k++] = (uint32_t)x; q = *end ? end + 1 : end; }
    if (k == POOL_TIERS) { bool ok = true; for (int i = 0; i < k; i++) ok = ok && v[i] >= 1 && v[i] <= 1000; if (ok) memcpy(SHARE, v, sizeof(v)); }
  }
  size_t fr = 0, tot = 0;
  hipError_t e = hipSuccess;
  uint64_t pool_bytes = pool_bytes_opt;
  if (!pool_bytes) { pool_bytes = 16ull << 30; if (hipMemGetInfo(&fr, &tot) == hipSuccess) { pool_bytes = (uint64_t)fr / 4; if (pool_bytes > (64ull << 30)) pool_bytes = 64ull << 30; if (pool_bytes < (1ull << 30)) pool_bytes = 1ull << 30; } }
  uint64_t caps[POOL_TIERS]; int nt = 0;
  for (uint64_t cap = work_cap; cap < big && nt < POOL_TIERS; ) { cap = (cap * 2 < big && nt < POOL_TIERS - 1) ? cap * 2 : big; caps[nt++] = cap; }   // the last tier always has the full size
  uint32_t share_sum = 0;
  for (int k = 0; k < nt; k++) share_sum += SHARE[k == nt - 1 ? POOL_TIERS - 1 : k];
  for (int k = 0; k < nt; k++) {
    uint64_t stride_t = (caps[k] + 255) & ~255ull;
    uint64_t cnt = pool_bytes / share_sum * SHARE[k == nt - 1 ? POOL_TIERS - 1 : k] / stride_t; if (cnt < 1) cnt = 1; if (cnt > 4096) cnt = 4096;
    if (ctx->cus < 64 && cnt > 2) cnt = 2;                                         // (the emulator)
    int t = pl->ntiers + 1;
    for (; cnt >= 1; cnt /= 2) { e = pl->base[t].grow(stride_t * cnt); if (e == hipSuccess) break; }
    if (e != hipSuccess) break;
    pl->stride[t] = stride_t; pl->cap[t] = caps[k]; pl->cnt[t] = (uint32_t)cnt; pl->ntiers++;
  }
  uint64_t nring = 4;
  for (int t = 1; t <= pl->ntiers; t++) nring += pl->cnt[t];
  std::vector<uint32_t> init(nring);
  PoolCounters ctr; memset(&ctr, 0, sizeof ctr);
  if (pl->d_rings.grow(nring) != hipSuccess || pl->d_ctr.grow(1) != hipSuccess) { pool_free(pl); ctx->err = "work-area pool: out of device memory"; return EH_E_NOMEM; }
  uint64_t o = 0;
  for (int t = 1; t <= pl->ntiers; t++) {
    pl->ring[t] = pl->d_rings + o;
    for (uint32_t k = 0; k < pl->cnt[t]; k++) init[o + k] = k;
    ctr.ring[t].pop = 0; ctr.ring[t].push = pl->cnt[t];
    o += pl->cnt[t];
  }
  if (hipMemcpy(pl->d_rings, init.data(), nring * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(pl->d_ctr, &ctr, sizeof ctr, hipMemcpyHostToDevice) != hipSuccess) { pool_free(pl); ctx->err = "work-area pool: hipMemcpy failed"; return EH_E_HIP; }
  if (pl->d_board.grow(1) != hipSuccess || hipMemset(pl->d_board, 0, sizeof(CoBoard)) != hipSuccess) { pool_free(pl); ctx->err = "work-area pool: no memory for the cooperation board"; return EH_E_NOMEM; }
  pl->refs = 1; g_pools.push_back(pl); ctx->pool = pl;
  return EH_OK;
}

// From which size a loop of a case is posted for other wavefronts, and in what chunks (KParams co_*).  A chunk costs its runner an
// agent-scope acquire and a release (microseconds, and the release writes back whatever is dirty in its XCD's L2), so chunks are
// hundreds of kilobytes; measurement knobs: EH_CO_COPY_MIN / EH_CO_COPY_CHUNK (bytes), EH_CO_FB_MIN / EH_CO_FB_CHUNK (positions).
static uint32_t co_env(const char* name, uint32_t dflt) { const char* v = getenv(name); if (!v || !*v) return dflt; unsigned long long x = strtoull(v, nullptr, 10); return x > 0 && x < (1ull << 31) ? (uint32_t)x : dflt; }
static void co_defaults(KParams* p, int cus) {
  const bool emu = cus < 64;                                                    // (the emulator's tests are small: they take the posted paths too)
  p->co_copy_min = co_env("EH_CO_COPY_MIN", emu ? (8u << 10) : (2u << 20));
  p->co_copy_chunk = co_env("EH_CO_COPY_CHUNK", emu ? (2u << 10) : (256u << 10));
  p->co_fb_min = co_env("EH_CO_FB_MIN", emu ? (16u << 10) : (512u << 10));
  p->co_fb_chunk = co_env("EH_CO_FB_CHUNK", emu ? (4u << 10) : (64u << 10)) & ~1023u;
  { const char* v = getenv("EH_CO_LINGER"); p->co_linger = v && *v ? (uint32_t)strtoul(v, nullptr, 10) : CO_LINGER; p->pad_co = 0; }
  if (p->co_copy_chunk < 1024) p->co_copy_chunk = 1024;
  if (p->co_fb_chunk < 1024) p->co_fb_chunk = 1024;
}

int eh_pool_stats(eh_ctx* ctx, uint64_t* out /* 64 values */) {
  if (!ctx || !out) return EH_E_INVALID;
  if (!ctx->pool) { ctx->err = "no work-area pool yet (eh_reserve or a first batch creates it)"; return EH_E_STATE; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  PoolCounters raw;
  HIPCHK(ctx, hipMemcpy(&raw, ctx->pool->d_ctr, sizeof raw, hipMemcpyDeviceToHost));   // (a plain copy: fine while batches run)
  memcpy(out, &raw, offsetof(PoolCounters, most_out));                                  // words [0, 40): rings, wait ticks, waits
  out[40] = (uint64_t)ctx->pool->ntiers;
  for (int t = 0; t <= POOL_TIERS; t++) {
    out[41 + t] = t >= 1 && t <= ctx->pool->ntiers ? (uint64_t)ctx->pool->cnt[t] | (raw.most_out[t] << 32) : 0;   // areas | the most that were out at once
    out[51 + t] = t <= ctx->pool->ntiers ? ctx->pool->cap[t] : 0;
  }
  out[61] = (uint64_t)ctx->pool->refs; out[62] = ctx->nslots; out[63] = 0;
  return EH_OK;
}
// Cooperative execution (eh_common.h CoBoard): out[0] loops posted, [1] chunks run by wavefronts between cases, [2] by the posting
// cases themselves, [3] cycles the posters waited for the last chunks, [4] loops that found the board full (run by their case alone).
int eh_coop_stats(eh_ctx* ctx, uint64_t* out /* 8 values */) {
  if (!ctx || !out) return EH_E_INVALID;
  if (!ctx->pool) { ctx->err = "no work-area pool yet (eh_reserve or a first batch creates it)"; return EH_E_STATE; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpy(out, (const uint8_t*)ctx->pool->d_board.p + offsetof(CoBoard, stat), sizeof(CoBoard::stat), hipMemcpyDeviceToHost));
  return EH_OK;
}
