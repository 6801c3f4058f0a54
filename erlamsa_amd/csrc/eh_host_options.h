// eh_host_options.h - host: the option strings (mutations, patterns, generators), eh_configure, the option profiles, and the entry
// points that only name things.
#pragma once
// erlamsa_utils:sort_by_priority/1 (erlamsa_utils.erl:113-117): lists:sort/2 with a strict '>' as the ordering fun — the
// order among equal priorities is whatever stdlib's merge sort gives (eh_otp_sort.h, the one implementation).
struct PItem { uint32_t pri; int id; };
typedef std::vector<PItem> PL;
static PL otp_sort_desc_strict(const PL& in) {
  otp::ListsSort<PItem> srt([](const PItem& a, const PItem& b) { return a.pri > b.pri; });
  return srt.sort(in);
}

static int lookup(const char* name, bool muta) {
  if (muta) { for (int i = 0; i < M_COUNT; i++) if (!strcmp(name, MUTAS[i].name)) return i; }
  else { for (int i = 0; i < P_COUNT; i++) if (!strcmp(name, PATS[i].name)) return i; }
  return -1;
}
// The "name[=pri],..." lists of -m, -p and -g: item(tok, name, pri) for every non-empty entry `tok`, `pri` the text behind its '=' or
// NULL; the first non-zero answer ends the walk and is returned.
template <class F> static int split_list(const char* s, F item) {
  std::string str(s); size_t pos = 0;
  while (pos <= str.size()) {
    size_t e = str.find(',', pos); if (e == std::string::npos) e = str.size();
    std::string tok = str.substr(pos, e - pos); pos = e + 1;
    if (tok.empty()) continue;
    size_t eq = tok.find('=');
    std::string name = eq == std::string::npos ? tok : tok.substr(0, eq);
    if (int rc = item(tok, name, eq == std::string::npos ? nullptr : tok.c_str() + eq + 1)) return rc;
  }
  return EH_OK;
}
// "-m"/"-p" list syntax: erlamsa_cmdparse:string_to_actions/3 (erlamsa_cmdparse.erl:232-257)
static int parse_actions(eh_ctx* ctx, const char* s, bool muta, std::vector<long>& pri /* -1 = not selected */) {
  int count = muta ? (int)M_COUNT : (int)P_COUNT;
  pri.assign(count, -1);
  if (!s) { for (int i = 0; i < count; i++) pri[i] = muta ? MUTAS[i].pri : PATS[i].pri; return EH_OK; }
  return split_list(s, [&](const std::string& tok, const std::string& name, const char* ptxt) {
    int id = lookup(name.c_str(), muta);
    if (id < 0) { ctx->err = std::string("No such ") + (muta ? "mutations" : "patterns") + ": " + name; return (int)EH_E_INVALID; }
    long p = muta ? MUTAS[id].pri : PATS[id].pri;
    if (ptxt) { char* endp = nullptr; p = strtol(ptxt, &endp, 10); if (*endp || p < 0 || p > 1000000) { ctx->err = "Invalid priority: " + tok; return (int)EH_E_INVALID; } }
    pri[id] = p;
    return (int)EH_OK;
  });
}
// -g: the generators that read no file or socket, with the priorities of erlamsa_gen:generators/0 where none is given.  The result is
// in that table's order (:250-257); *needs_paths = the corpus entries they need (file: 1, jump: 2).  A priority is read as it comes.
static int parse_generators(eh_ctx* ctx, const char* s, PL& gl, int* needs_paths) {
  long gr = 1, gd = 500, gf = -1, gj = -1;
  if (s) {
    gr = -1; gd = -1;
    int rc = split_list(s, [&](const std::string&, const std::string& name, const char* ptxt) {
      long p = ptxt ? strtol(ptxt, nullptr, 10) : -1;
      if (name == "random") gr = p < 0 ? 1 : p; else if (name == "direct") gd = p < 0 ? 500 : p;
      else if (name == "file") gf = p < 0 ? 1000 : p; else if (name == "jump") gj = p < 0 ? 100 : p;      // Paths = the corpus entries
      else { ctx->err = "generator '" + name + "' is host-side I/O and not part of the GPU path"; return (int)EH_E_UNSUPPORTED; }
      return (int)EH_OK;
    });
    if (rc) return rc;
  }
  if (gr >= 0) gl.push_back({(uint32_t)gr, G_RANDOM});
  if (gj >= 0) gl.push_back({(uint32_t)gj, G_JUMP});
  if (gd >= 0) gl.push_back({(uint32_t)gd, G_DIRECT});
  if (gf >= 0) gl.push_back({(uint32_t)gf, G_FILE});
  *needs_paths = gj >= 0 ? 2 : (gf >= 0 ? 1 : 0);
  return EH_OK;
}

// The part of the option map a PROFILE owns - mutations, patterns, blockscale - parsed as erlamsa_main:fuzzer/1 reads them
// (erlamsa_main.erl:127-163).  eh_configure and eh_profile_add both come through here, so a profile is the context's configuration
// bit for bit when the strings are the same.  `pc` is written only on success and has no uninitialised byte (profiles are interned
// by their bytes).
static int parse_profile(eh_ctx* ctx, const char* mutations, const char* patterns, double blockscale, ProfileCfg& pc) {
  ProfileCfg cfg;
  memset(&cfg, 0, sizeof(cfg));
  std::vector<long> mp, pp;
  int rc = parse_actions(ctx, mutations, true, mp); if (rc) return rc;
  rc = parse_actions(ctx, patterns, false, pp); if (rc) return rc;
  for (int i = 0; i < M_COUNT; i++) if (mp[i] >= 0) {
    if (!MUTAS[i].on_gpu) { ctx->err = std::string("mutator '") + MUTAS[i].name + "' is not available on the GPU in this build"; return EH_E_UNSUPPORTED; }
    cfg.sel_name[cfg.nsel] = (uint8_t)i; cfg.sel_pri[cfg.nsel] = (uint32_t)mp[i]; cfg.nsel++;
  }
  // make_pattern (erlamsa_patterns.erl:416-428): foldl prepends => reversed table order, then sort_by_priority
  PL pl;
  for (int i = P_COUNT - 1; i >= 0; i--) if (pp[i] >= 0) {
    if (!PATS[i].on_gpu) { ctx->err = std::string("pattern '") + PATS[i].name + "' is not available on the GPU in this build"; return EH_E_UNSUPPORTED; }
    pl.push_back({(uint32_t)pp[i], i});
  }
  PL sp = otp_sort_desc_strict(pl);
  cfg.npat = (int)sp.size();
  for (size_t i = 0; i < sp.size(); i++) { cfg.pat_id[i] = (uint8_t)sp[i].id; cfg.pat_pri[i] = sp[i].pri; cfg.pat_total += (int)sp[i].pri; }
  if (cfg.npat == 0) { ctx->err = "no patterns selected"; return EH_E_INVALID; }
  double bs = blockscale == 0 ? 1.0 : blockscale;
  cfg.max_block_scaled = (uint32_t)llround(MAX_BLOCK_SIZE * bs);
  cfg.min_block_scaled = (uint32_t)llround(MIN_BLOCK_SIZE * bs);
  pc = cfg;
  return EH_OK;
}
static std::string profile_key(const ProfileCfg& pc) { return std::string((const char*)&pc, sizeof(pc)); }

int eh_configure(eh_ctx* ctx, const eh_options* o) {
  if (!ctx || !o) return EH_E_INVALID;
  if (o->abi_version != EH_ABI_VERSION) { ctx->err = "eh_options.abi_version mismatch"; return EH_E_INVALID; }
  // Requests that are still PENDING run with the configuration in force when they are launched, so a new one is refused
  // (eh_flush them first).  A batch that is already in flight carries its configuration with it (launch() copies it into the
  // kernel's argument block) but owns the context's result buffers, which the next launch may re-size: it is collected first.
  std::unique_lock<std::mutex> lk(ctx->co_lock);
  if (ctx->co.pending.size()) {
    ctx->err = "coalesced requests are pending on this context: eh_flush them first, or use a context of its own";
    return EH_E_STATE;
  }
  if (ctx->co.in_flight) { int rcc = co_collect(ctx, lk); if (rcc) return rcc; }
  if (o->sequence_muta) {
    ctx->err = "sequence_muta (--consequtive-mutators, erlamsa_main.erl:223-235) chains the mutator scores from case to case: a batch of independent cases cannot keep that order; route this run to the BEAM path";
    return EH_E_UNSUPPORTED;
  }
  DevConfig cfg;
  memset(&cfg, 0, sizeof(cfg));
  ProfileCfg p0;
  int rc = parse_profile(ctx, o->mutations, o->patterns, o->blockscale, p0); if (rc) return rc;
  cfg.nsel = p0.nsel; memcpy(cfg.sel_name, p0.sel_name, sizeof(cfg.sel_name)); memcpy(cfg.sel_pri, p0.sel_pri, sizeof(cfg.sel_pri));
  cfg.npat = p0.npat; cfg.pat_total = p0.pat_total; memcpy(cfg.pat_id, p0.pat_id, sizeof(cfg.pat_id)); memcpy(cfg.pat_pri, p0.pat_pri, sizeof(cfg.pat_pri));
  cfg.max_block_scaled = p0.max_block_scaled; cfg.min_block_scaled = p0.min_block_scaled;
  PL gl;
  rc = parse_generators(ctx, o->generators, gl, &ctx->needs_paths); if (rc) return rc;
  if (gl.empty()) { ctx->err = "No generators!"; return EH_E_INVALID; }
  PL sg = otp_sort_desc_strict(gl);
  cfg.ngen = (int)sg.size();
  for (size_t i = 0; i < sg.size(); i++) { cfg.gen_id[i] = (uint8_t)sg[i].id; cfg.gen_pri[i] = sg[i].pri; cfg.gen_total += (int)sg[i].pri; }
  snprintf(cfg.ssrf_host, sizeof(cfg.ssrf_host), "%s", o->ssrf_host ? o->ssrf_host : "localhost");
  snprintf(cfg.ssrf_port, sizeof(cfg.ssrf_port), "%d", o->ssrf_port ? o->ssrf_port : 51234);
  // all profiles go, their ids with them; profile 0 is this configuration
  try {
    std::vector<ProfileCfg> one(1, p0); std::unordered_map<std::string, uint32_t> idx; idx.emplace(profile_key(p0), 0u);
    ctx->profiles.list.swap(one); ctx->profiles.index.swap(idx);
  } catch (const std::bad_alloc&) { ctx->err = "out of host memory"; return EH_E_NOMEM; }
  ctx->profiles.on_device = 0;
  ctx->cfg = cfg;
  ctx->work_budget = o->max_case_work;
  ctx->big_case_bytes = o->big_case_bytes; ctx->max_case_bytes = o->max_case_bytes; ctx->out_capacity_opt = o->out_capacity; ctx->max_slots_opt = o->max_slots; ctx->flags = o->flags;
  ctx->fuse_stream_min = o->fuse_stream_min ? o->fuse_stream_min : 16384;
  ctx->pool_bytes_opt = o->pool_bytes; ctx->dl_chunk = o->download_chunk_bytes ? o->download_chunk_bytes : (256ull << 20);
  ctx->configured = true;
  return EH_OK;
}

// ---- option profiles ----------------------------------------------------------------------------------------
int eh_profile_add(eh_ctx* ctx, const char* mutations, const char* patterns, double blockscale, uint32_t* id) {
  if (!ctx || !id) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock);
  if (!ctx->configured) { ctx->err = "configure first"; return EH_E_STATE; }
  ProfileCfg pc;
  int rc = parse_profile(ctx, mutations, patterns, blockscale, pc);
  if (rc) return rc;
  try {
    const std::string key = profile_key(pc);
    auto it = ctx->profiles.index.find(key);
    if (it != ctx->profiles.index.end()) { *id = it->second; return EH_OK; }
    if (ctx->profiles.list.size() >= MAX_PROFILES) { ctx->err = "the profile table is full (EH_MAX_PROFILES = " + std::to_string(MAX_PROFILES) + "): eh_configure starts a new one"; return EH_E_NOMEM; }
    ctx->profiles.list.reserve(ctx->profiles.list.size() + 1);
    ctx->profiles.index.emplace(key, (uint32_t)ctx->profiles.list.size());
    ctx->profiles.list.push_back(pc);                          // (room reserved above: cannot throw)
  } catch (const std::bad_alloc&) { ctx->err = "out of host memory"; return EH_E_NOMEM; }
  *id = (uint32_t)ctx->profiles.list.size() - 1;
  return EH_OK;
}
int eh_profile_count(eh_ctx* ctx, uint32_t* n) {
  if (!ctx || !n) return EH_E_INVALID;
  std::lock_guard<std::mutex> g(ctx->co_lock);
  *n = (uint32_t)ctx->profiles.list.size();
  return EH_OK;
}

uint32_t eh_abi_version(void) { return EH_ABI_VERSION; }
int eh_mutator_count(void) { return M_COUNT; }
const char* eh_mutator_name(int id) { return id >= 0 && id < M_COUNT ? MUTAS[id].name : nullptr; }
int eh_mutator_default_pri(int id) { return id >= 0 && id < M_COUNT ? MUTAS[id].pri : -1; }
int eh_mutator_on_gpu(int id) { return id >= 0 && id < M_COUNT ? MUTAS[id].on_gpu : 0; }
int eh_pattern_count(void) { return P_COUNT; }
const char* eh_pattern_name(int id) { return id >= 0 && id < P_COUNT ? PATS[id].name : nullptr; }
int eh_pattern_default_pri(int id) { return id >= 0 && id < P_COUNT ? PATS[id].pri : -1; }
int eh_pattern_on_gpu(int id) { return id >= 0 && id < P_COUNT ? PATS[id].on_gpu : 0; }
const char* eh_kernel_name(void) { return "eh_mutate_kernel"; }
int eh_meta_atom_count(void) { return AT_COUNT; }
const char* eh_meta_atom_name(int id) {
  static const char* const names[AT_COUNT] = {
#define EH_ATOM_NAME(n) #n,
      EH_ATOMS(EH_ATOM_NAME)
#undef EH_ATOM_NAME
  };
  return id >= 0 && id < AT_COUNT ? names[id] : nullptr;
}

const char* eh_strerror(int code) {
  switch (code) {
    case EH_OK: return "ok";
    case EH_E_INVALID: return "invalid argument";
    case EH_E_NODEVICE: return "no usable HIP device";
    case EH_E_HIP: return "HIP runtime error";
    case EH_E_NOMEM: return "out of memory";
    case EH_E_STATE: return "wrong call order";
    case EH_E_AGAIN: return "request not launched yet";
    case EH_E_UNSUPPORTED: return "mutator/pattern not available on the GPU in this build";
  }
  return "unknown error";
}
const char* eh_last_error(eh_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }
uint64_t eh_last_error_copy(eh_ctx* ctx, char* buf, uint64_t cap) {
  if (!buf || !cap) return 0;
  if (!ctx) { buf[0] = 0; return 0; }
  std::lock_guard<std::mutex> g(ctx->co_lock);                      // the coalescer's calls set the text under this lock
  uint64_t n = ctx->err.size() < cap - 1 ? ctx->err.size() : cap - 1;
  memcpy(buf, ctx->err.data(), n); buf[n] = 0;
  return n;
}
