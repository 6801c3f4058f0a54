// eh_host.h - host side of liberlamsa_hip.so: the tables of names, the owner of a device buffer, the context and the guards that
// entry points open with.  The eh_host_*.h files are parts of eh_engine.hip's translation unit, included there in an order that
// needs no forward declaration; the entry points take their C linkage from their declarations in include/erlamsa_hip.h.
#pragma once
using namespace eh;

static const MutaInfo MUTAS[M_COUNT] = {
    {"sgm", 10, 1}, {"js", 3, 1},  {"uw", 1, 1},   {"ui", 2, 1},  {"ab", 1, 1},  {"ad", 1, 1},  {"tr2", 1, 1}, {"td", 1, 1},
    {"num", 3, 1},  {"ts1", 2, 1}, {"tr", 2, 1},   {"ts2", 2, 1}, {"bd", 1, 1},  {"bei", 1, 1}, {"bed", 1, 1}, {"bf", 1, 1},
    {"bi", 1, 1},   {"ber", 1, 1}, {"br", 1, 1},   {"sp", 1, 1},  {"sr", 1, 1},  {"sd", 1, 1},  {"snand", 1, 1}, {"srnd", 1, 1},
    {"ld", 1, 1},   {"lds", 1, 1}, {"lr2", 1, 1},  {"lri", 1, 1}, {"lr", 1, 1},  {"ls", 1, 1},  {"lp", 1, 1},  {"lis", 1, 1},
    {"lrs", 1, 1},  {"ft", 2, 1},  {"fn", 1, 1},   {"fo", 2, 1},  {"len", 2, 1}, {"b64", 7, 1}, {"uri", 1, 1}, {"zip", 1, 1},
    {"nil", 0, 1}};
static const PatInfo PATS[P_COUNT] = {{"od", 1, 1}, {"nd", 2, 1}, {"bu", 1, 1}, {"sk", 2, 1}, {"sz", 2, 1},
                                      {"cs", 1, 1}, {"ar", 1, 1}, {"cp", 1, 1}, {"co", 0, 1}, {"nu", 0, 1}};

// Host code fills KParams.  In the device pass of this file its pointer members are address-space qualified (eh_common.h), and
// the host functions are type-checked there too: dp(x) converts to whatever the member is.
template <class T> struct DevPtr { T* p; template <class U> operator U() const { return (U)p; } };
template <class T> static inline DevPtr<T> dp(T* p) { return DevPtr<T>{p}; }

// The owner of a device allocation, and the only place of the host side that allocates or frees device memory: the pointer and its
// capacity (in elements) change only together, so after a failed growth the buffer is empty, not stale.  Contents are never kept.
template <class T> struct DevBuf {
  T* p = nullptr;
  uint64_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
  }
  hipError_t reset(uint64_t n) {                        // exactly n elements, whatever it held
    release();
    hipError_t e = hipMalloc(&p, n * sizeof(T));
    if (e == hipSuccess) cap = n; else p = nullptr;
    return e;
  }
  hipError_t grow(uint64_t n) { return n <= cap ? hipSuccess : reset(n); }
  void swap(DevBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
  operator T*() const { return p; }
};
template <class T> static inline DevPtr<T> dp(const DevBuf<T>& b) { return DevPtr<T>{b.p}; }

// the work-area pool of a device (see pool_acquire)
struct DevPool {
  int device = 0; uint64_t work_cap = 0, big = 0, pool_bytes_opt = 0;
  int refs = 0;
  int ntiers = 0;                                       // tiers 1..ntiers
  DevBuf<uint8_t> base[POOL_TIERS + 1]; uint64_t stride[POOL_TIERS + 1] = {}, cap[POOL_TIERS + 1] = {}; uint32_t cnt[POOL_TIERS + 1] = {};
  DevBuf<uint32_t> d_rings; uint32_t* ring[POOL_TIERS + 1] = {}; DevBuf<PoolCounters> d_ctr;
  DevBuf<CoBoard> d_board;                              // cooperative execution: the board every context of the device posts on (eh_common.h)
};

// ---- the parts of a context: each owns what it holds - device memory through DevBuf, events, streams and page-locked memory
// through its own destructor.  Nothing is released by hand: eh_destroy synchronises the device and deletes the context.
// The current corpus, in the context's own buffers (upload, collectives: reused while they fit) or the caller's (eh_corpus_attach).
struct Corpus {
  uint8_t* d = nullptr; uint64_t* d_off = nullptr;
  DevBuf<uint8_t> own; DevBuf<uint64_t> own_off;
  uint64_t n = 0, bytes = 0;
  std::vector<uint64_t> h_off;   // host copy of offsets (for totals)
};
// Option profiles (eh_profile_add), guarded by co_lock.  list[0] = what eh_configure was given; entries are never changed once made,
// ids only grow until the next eh_configure.  The device table has room for all EH_MAX_PROFILES; entries [0, on_device) of it
// are current, the rest is copied before the next profiled launch (launches of one context run one after the other).
struct Profiles {
  std::vector<ProfileCfg> list; std::unordered_map<std::string, uint32_t> index;
  DevBuf<ProfileCfg> d_table; uint32_t on_device = 0;
};
// What a launch writes and the result calls read: the arenas, an entry per case in each of the result arrays, and the last batch.
struct Results {
  DevBuf<uint8_t> d_out;
  DevBuf<uint8_t> d_out2;                               // EH_FLAG_ORDERED_OUTPUT: second arena (case order)
  DevBuf<uint64_t> d_ord;                               // ordered offsets (n + 1)
  bool ordered = false;                                 // the last batch's results are in case order
  DevBuf<uint64_t> d_off, d_len, d_draws, d_cycles, d_peak, d_toff;
  DevBuf<int32_t> d_status, d_lastm;
  DevBuf<uint32_t> d_tlen;
  DevBuf<BatchCounters> d_counters;                     // one: the batch's counters (eh_common.h)
  DevBuf<KParams> d_params;                             // argument block of eh_mutate_kernel
  DevBuf<RunState> d_run;
  DevBuf<uint8_t> d_seeds;                              // mode 1, SEED_ROW bytes per case: three int64 seeds for every case, then a uint32 profile id for every case
  BatchSummary* h_sum = nullptr; uint64_t batch_seq = 0;   // page-locked: the last batch's totals, written by the kernel (KParams::summary_out)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;              // around eh_mutate_kernel (eh_create)
  hipStream_t last_stream = nullptr;
  hipStream_t own_stream = nullptr;                     // eh_stream: a stream of the context's own (non-blocking), made on first request
  uint64_t last_n = 0, last_in_bytes = 0;
  bool have_result = false;
  ~Results() {
    if (h_sum) (void)hipHostFree(h_sum);
    if (own_stream) (void)hipStreamDestroy(own_stream);
    if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1);
  }
};
// eh_result_download: case-ordered chunks are gathered on the device into two bounce buffers; chunk k goes over PCIe
// while chunk k+1 is gathered
struct Downloader {
  DevBuf<uint8_t> bounce[2]; uint64_t chunk = 0; hipStream_t gather = nullptr, copy = nullptr;
  hipEvent_t ev_g[2] = {nullptr, nullptr}, ev_c[2] = {nullptr, nullptr};
  DevBuf<uint64_t> d_sel;                               // eh_result_download_select: offsets, lengths, destinations of the listed cases
  ~Downloader() {
    for (int k = 0; k < 2; k++) { if (ev_g[k]) (void)hipEventDestroy(ev_g[k]); if (ev_c[k]) (void)hipEventDestroy(ev_c[k]); }
    if (gather) (void)hipStreamDestroy(gather); if (copy) (void)hipStreamDestroy(copy);
  }
};
// uniqueness filter (eh_unique.h): sized on first use, reused while they fit; results are cached per batch (Results::batch_seq)
struct UniqueState {
  DevBuf<uint64_t> d_digest, d_first, d_pfirst; DevBuf<uint32_t> d_flag;
  DevBuf<unsigned long long> d_term;                                         // a pair of CRCs per piece
  DevBuf<unsigned long long> d_tab;                                          // [0] unique cases, [1] their bytes, then owner[slots], rep[slots]
  uint64_t digest_seq = 0, unique_seq = 0, n_unique = 0, bytes = 0;          // batch the device arrays / the two totals belong to (0: none)
};
// seen set (eh_seen.h): made by eh_seen_reserve, kept across batches, corpus uploads and eh_configure.  The classification of a batch is
// cached like the filter's results (seq), and so is whether its keys have been recorded
struct SeenState {
  DevBuf<uint64_t> d_keys, d_pos; DevBuf<unsigned long long> d_tab, d_ctr; DevBuf<uint8_t> d_cls;
  uint64_t capacity = 0, slots = 0, held = 0, dropped = 0; bool have = false;
  uint64_t seq = 0, n_fresh = 0, fresh_bytes = 0; bool committed = false;
  void reset() {                                                             // no set
    d_keys.release(); d_tab.release(); d_ctr.release(); d_pos.release(); d_cls.release();
    capacity = slots = held = dropped = seq = 0; have = false; committed = false;
  }
};
// corpus promotion (eh_promote.h): sized on first use, reused while they fit.  `ent` holds the three entry arrays one behind the other
// (source offsets, lengths, destinations: `ent_cap` entries each), `elen` a value per case of the batch, `pfirst` a piece number per entry
struct PromoteState {
  DevBuf<uint64_t> d_elen, d_ent, d_pfirst; DevBuf<unsigned long long> d_ctr;
  uint64_t ent_cap = 0;
};

struct eh_ctx {
  int device = 0;
  int cus = 0;
  std::string err;
  bool configured = false;
  DevConfig cfg;
  uint64_t max_case_bytes = 0, out_capacity_opt = 0, work_budget = 0;
  uint64_t fuse_stream_min = 16384, pool_bytes_opt = 0, dl_chunk = 256ull << 20;   // eh_options (ABI 4)
  uint32_t max_slots_opt = 0, flags = 0;
  int needs_paths = 0;                                  // corpus entries the configured generators need (file: 1, jump: 2)
  uint64_t big_case_bytes = 0;
  // work areas: a pool shared by every context of the device with the same sizes (DevPool above)
  DevPool* pool = nullptr;
  DevBuf<uint8_t> d_slots; uint64_t slot_stride = 0, slot_cap = 0; uint32_t nslots = 0;   // a slot per workgroup of a batch
  Corpus corpus;
  Profiles profiles;
  Results res;
  Downloader dl;
  UniqueState uq;
  SeenState sn;
  PromoteState pm;
  // request coalescing (eh_submit / eh_flush / eh_poll): the bookkeeping (eh_coalesce.h) and its lock, which a public entry point takes
  // once and no function below it takes again
  Coalescer co; std::mutex co_lock;
  std::condition_variable co_cv; bool co_collecting = false;       // a thread is waiting for / downloading the in-flight batch (lock released)
  void* comm = nullptr; int comm_rank = 0, comm_n = 1;   // RCCL communicator of this context's device (eh_comm_init / eh_comm_init_local)
};

#define HIPCHK(ctx, call)                                                                             \
  do {                                                                                                \
    hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess) {                                                                           \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                                 \
      return EH_E_HIP;                                                                                \
    }                                                                                                 \
  } while (0)

// A context that has coalesced requests pending or in flight (eh_submit .. eh_poll) belongs to the coalescer: a batch,
// a corpus or a configuration from outside would overwrite the buffers and options those requests run with.  What those entry
// points ask first, co_lock held (the coalescer itself calls the functions below them, which do not ask).
static int co_idle(eh_ctx* ctx) {
  if (!ctx->co.busy()) return EH_OK;
  ctx->err = "coalesced requests are pending on this context: eh_flush and eh_poll them first, or use a context of its own";
  return EH_E_STATE;
}

// What the calls that read the last batch's results begin with: there is one and (`wait`) it has ended.  Without `wait` the caller
// has checks of its own, or a cheaper way to learn that the batch has ended, in front of its eh_sync.
static int result_ready(eh_ctx* ctx, bool wait = true) {
  if (!ctx->res.have_result) { ctx->err = "no batch has run"; return EH_E_STATE; }
  return wait ? eh_sync(ctx) : EH_OK;
}
// What the calls that use the context's streams and arrays for work of their own go on with once their arguments are checked: the
// device is current and the last batch, if there was one, has ended.  (co_idle comes first in each of them, as in every entry point.)
static int device_quiet(eh_ctx* ctx) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return ctx->res.have_result ? eh_sync(ctx) : EH_OK;
}
// The results derived from a batch are cached under its number (Results::batch_seq): the filter's arrays (digests, first_of, flags,
// the two totals) and the seen set's classification (cls, pos, the fresh totals).  Whoever is about to overwrite those arrays with
// values of something else - a caller-made arena, the corpus, a list of keys - or to change the set itself says so here first.
enum : unsigned { DERIVED_FILTER = 1, DERIVED_SEEN = 2 };
static void invalidate_derived(eh_ctx* ctx, unsigned which) {
  if (which & DERIVED_FILTER) ctx->uq.digest_seq = ctx->uq.unique_seq = 0;
  if (which & DERIVED_SEEN) ctx->sn.seq = 0;
}
