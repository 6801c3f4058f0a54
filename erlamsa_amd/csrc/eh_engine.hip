// eh_engine.hip — the one translation unit of liberlamsa_hip.so: the kernels here, the patterns and generators they run in
// eh_patterns.h / eh_gen.h, and the C ABI (include/erlamsa_hip.h) in the eh_host*.h files included at the end.
//
// Kernels (gfx950 only):
//   eh_prologue_kernel: counters + argument block of a batch, per-run setup of erlamsa_main:fuzzer/1 (one wavefront)
//   eh_mutate_kernel  : persistent grid, one wavefront per case, cases pulled from a ticket
//                       counter; runs generator -> pattern -> mux_fuzzers -> mutators and
//                       writes each case's output into a bump-allocated arena.
//
// Reference call path restated here (src/ of the reference):
//   erlamsa_main.erl:125-247  fuzzer/1 (setup draw order, per-case ThreadSeed, worker body)
//   erlamsa_gen.erl:43-56,152-199  finish/1, direct_generator/2, random_stream/1, mux_generators/2
//   erlamsa_patterns.erl:45-60,146-161,265-442  split, skipper, mutate_once(_loop), od/nd/bu/co/nu, mux_patterns
//   erlamsa_mutations.erl  (see eh_device.h)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <map>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <string>
#include <vector>

#include "../../include/erlamsa_hip.h"
#include "eh_otp_sort.h"
#include "eh_device.h"
#include "eh_text.h"
#include "eh_lex.h"
#include "eh_tree.h"
#include "eh_field.h"
#include "eh_fuse.h"
#include "eh_fuse2.h"
#include "eh_doc.h"
#include "eh_sgml.h"
#include "eh_json.h"
#include "eh_zlib.h"
#include "eh_zip.h"
#include "eh_unique.h"
#include "eh_seen.h"
#include "eh_promote.h"
#include "eh_comm.h"
#include "eh_coalesce.h"

namespace eh {


EH_DEV int run_mutator_ext(Ctx& c, uint32_t fn, uint32_t mask) {
  (void)mask;
  EH_G StState* st = c.aux->nest.st;
  switch (fn) {
    case M_LD: case M_LDS: case M_LR2: case M_LRI: case M_LR: case M_LS: case M_LP: return muta_line(c, (int)fn);
    case M_LIS: return muta_st_line(c, (int)fn, st);
    case M_LRS: return muta_st_line(c, (int)fn, st + 1);
    case M_NUM: return muta_num(c);
    case M_AB: case M_AD: return muta_ascii(c, lex_slot(c), (int)fn);
    case M_URI: return muta_uri(c, lex_slot(c));
    case M_B64: return muta_b64(c, lex_slot(c));
    case M_ZIP: return muta_zip(c);
    case M_LEN: return muta_len(c);
    case M_FT: case M_FN: case M_FO: return muta_fuse(c, (int)fn, &c.aux->nest.fo);
    case M_TR2: case M_TD: case M_TS1: case M_TS2: case M_TR: return muta_tree(c, (int)fn);
    case M_SGM: return muta_sgml(c);
    case M_JS: return muta_json(c);
    default: c.status = CASE_UNSUPPORTED; c.r_kind = R_SAME; return 0;
  }
}

// =============================================================================================
// device: per-run setup  (erlamsa_main.erl:134-158)
// =============================================================================================
// `sel` holds the selected mutators (nsel, sel_name, sel_pri): the context's DevConfig or, for a case of a profiled launch, its
// ProfileCfg; `cfg` holds the generators.  Both are template parameters so that each keeps the address space it is passed with
// (kernel argument or global memory): one generic reference for the two would turn the table loads into flat_* instructions.
template <class Sel, class Gen>
EH_DEV void setup_run(const Sel& sel, const Gen& cfg, int64_t s1, int64_t s2, int64_t s3, Rng& rng, int& gen, int& snand_mask,
                      uint32_t& e_pri, uint32_t& e_meta, int& nfs) {
  const int l = EH_LANE;
  rng.draws = 0;
  rng_seed(rng, s1, s2, s3);                                   // erlamsa_rnd:seed/1 :134
  // mutations/1 evaluates construct_sed_bytes_randmask twice: rand_elem over 3, then over 1 funs
  snand_mask = (int)rng_rand(rng, 3);                          // erlamsa_mutations.erl:311-312,1313
  (void)rng_rand(rng, 1);                                      // :1314
  // make_mutator (:1370-1383): Mutas = selected entries in REVERSE table order;
  // mutators_mutator (:1391-1395) draws rand(10) along that list and prepends => list in table order.
  nfs = sel.nsel;
  uint32_t score = 0;
  if (l < nfs) {
    double u = rng_peek(rng, (uint32_t)(nfs - 1 - l) + 1);
    uint32_t n = (uint32_t)(u * 10.0);
    score = n < 2 ? 2 : n;
  }
  rng_skip(rng, (uint64_t)nfs);
  uint32_t name = l < nfs ? sel.sel_name[l] : 0;
  e_pri = l < nfs ? sel.sel_pri[l] : 0;
  uint32_t mask = name == M_SNAND ? (uint32_t)snand_mask : 3u;
  e_meta = em_pack(score, name, name, mask);
  // mux_generators (erlamsa_gen.erl:194-199): rand(N) over the priority-sorted list
  uint32_t g = rng_rand(rng, (uint32_t)cfg.gen_total);
  gen = cfg.gen_id[cfg.ngen - 1];
  for (int i = 0; i < cfg.ngen; i++) {                         // choose_pri erlamsa_utils.erl:155-161
    if (g == 0 || g < cfg.gen_pri[i]) { gen = cfg.gen_id[i]; break; }
    g -= cfg.gen_pri[i];
  }
}
struct SelView { int32_t nsel; const EH_G uint8_t* sel_name; const EH_G uint32_t* sel_pri; };   // the `sel` of a mode-1 case: the context's tables or its profile's, global memory either way
// choose_pattern_fun (erlamsa_patterns.erl:431-434) + choose_pri over the priority-sorted patterns of `t` (DevConfig or ProfileCfg); -1: none
template <class Pats>
EH_DEV int choose_pattern(const Pats& t, Rng& rng) {
  uint32_t r = rng_rand(rng, (uint32_t)t.pat_total);
  int pat = t.npat > 0 ? t.pat_id[t.npat - 1] : -1;
  for (int k = 0; k < t.npat; k++) {
    if (r == 0 || r < t.pat_pri[k]) { pat = t.pat_id[k]; break; }
    r -= t.pat_pri[k];
  }
  return pat;
}

// One wavefront in front of every eh_mutate_kernel: the batch's counters back to zero, its argument block written to device memory,
// and (mode 0) the run state of the parent seed.  The runtime's own fill and copy kernels (hipMemsetAsync, hipMemcpyAsync from
// pageable memory) are workgroups of 256 work-items: four wavefronts that must find room on ONE compute unit at the same moment.
// On a device whose every slot is held by the one-wavefront workgroups of the passes in flight, and whose freed slots go to the
// next of those one at a time, they starve - 0.17 s on average and up to 0.8 s per launch with six passes in flight, seconds with
// twelve (profiles/r05_kernel_stats_before_prologue.csv) - and the pass behind them with them.  A one-wavefront kernel takes the
// next free slot like any other workgroup of the batch (the old eh_setup_kernel: 29 us on average in the same trace).
__global__ void __launch_bounds__(64) eh_prologue_kernel(KParams p, int64_t s1, int64_t s2, int64_t s3, RunState* out_, KParams* params_out_,
                                                         unsigned long long* counters_) {
  // (kernel arguments are what the host passes: generic pointers; counters_ is a BatchCounters, handed over as the words it is zeroed by)
  EH_G RunState* out = (EH_G RunState*)out_; EH_G KParams* params_out = (EH_G KParams*)params_out_; EH_G BatchCounters* counters = (EH_G BatchCounters*)counters_;
  const int l = EH_LANE;
  for (int i = l; i < (int)(sizeof(BatchCounters) / 8); i += 64) ((EH_G unsigned long long*)counters)[i] = 0;   // every word of the batch's counters
#ifdef EH_PROF
  if (l == 0) counters->prof[2 * PROF_WG_START] = ~0ull;         // earliest workgroup start: atomicMin
#endif
  static_assert(sizeof(KParams) % 4 == 0, "KParams is copied word by word");
  cwptr src = (cwptr)&p;
  wptr dst = (wptr)params_out;
  for (int i = l; i < (int)(sizeof(KParams) / 4); i += 64) dst[i] = src[i];
  if (p.mode != 0) return;
  Rng rng; int gen, mask, nfs; uint32_t e_pri, e_meta;
  setup_run(p.cfg, p.cfg, s1, s2, s3, rng, gen, mask, e_pri, e_meta, nfs);
  if (l == 0) { out->a1 = rng.a1; out->a2 = rng.a2; out->a3 = rng.a3; out->gen = gen; out->nfs = nfs; out->snand_mask = mask; }
  if (l < nfs) { out->fs_name[l] = (uint8_t)em_name(e_meta); out->fs_score[l] = (uint8_t)em_score(e_meta); out->fs_pri[l] = e_pri; }
}

#include "eh_patterns.h"
#include "eh_gen.h"

// =============================================================================================
// cooperative execution: chunk t of a posted loop (eh_device.h co_run / co_help)
// =============================================================================================
__device__ __noinline__ void co_exec(const EH_G CoJob* j, uint32_t t) {
  const uint32_t kind = uni(co_ld32(&j->kind));
  const uint64_t a0 = uni64(j->a[0]), a1 = uni64(j->a[1]), a2 = uni64(j->a[2]);
  if (kind == CO_COPY || kind == CO_EQUAL) {
    const uint32_t ch = uni((uint32_t)j->a[3]);
    const uint64_t off = (uint64_t)t * ch;
    const uint32_t len = a2 - off < ch ? (uint32_t)(a2 - off) : ch;
    if (kind == CO_COPY) wave_copy_raw((bptr)a0 + off, (cbptr)a1 + off, len);
    else if (!wave_equal_raw((cbptr)a0 + off, (cbptr)a1 + off, len)) { if (EH_LANE == 0) atomicAdd((EH_G unsigned long long*)&j->acc, 1ull); }
    return;
  }
  if (kind == CO_FBPASS) { fb_pass_chunk(j, t); return; }
}

// =============================================================================================
// the mutate kernel
// =============================================================================================
EH_DEV void sys_store(EH_G unsigned long long* p, unsigned long long v) {   // a store the host sees (page-locked host memory)
#ifdef HIPEMU
  *p = v;
#else
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#endif
}
constexpr unsigned int CO_LINGER = 24;       // wavefronts of a pass that stay for posted chunks once the pass is out of tickets
// 2 wavefronts per SIMD = up to 256 VGPRs: at 4 (128 VGPRs) the scheduler loops and the candidate loop of base64_mutator
// reload spilled registers from scratch on every iteration (7.5 M instead of 1.6 M memory instructions for one
// b64-heavy case, twice the time, profiles/r03_summary.json "occupancy"); the longest cases set the duration of a pass.
#ifndef EH_WAVES_PER_SIMD
#define EH_WAVES_PER_SIMD 2
#endif
// The argument block lives in device memory: taking the address of a by-value kernel argument (c.p) made the
// compiler keep a ~700-byte private copy of it per lane.
__global__ void __launch_bounds__(64, EH_WAVES_PER_SIMD) eh_mutate_kernel(const KParams* __restrict__ pp_) {
  const EH_G KParams* pp = (const EH_G KParams*)pp_;
  const int l = EH_LANE;
  const EH_G KParams& p = *pp;
  Ctx& c = g_ctx;
  LaneTab lt;
  c.p = pp;
  c.work_budget = p.work_budget;
#ifdef EH_PROF
  // how many workgroups the device holds at once: earliest / latest workgroup start of the dispatch (100 MHz wall clock)
  if (l == 0) { unsigned long long t = __builtin_amdgcn_s_memrealtime(); atomicMin(&pp->prof[2 * PROF_WG_START], t ? t : 1ull); atomicMax(&pp->prof[2 * PROF_WG_START + 1], t); }
#endif
  // this workgroup's slot: block tables + work area
  const uint32_t slot_id = blockIdx.x;
  EH_G Slot* slot = (EH_G Slot*)(p.slot_base + (uint64_t)slot_id * p.slot_stride);
  c.bl = slot->bl;
  c.bl2 = slot->bl2;
  c.em = slot->em;
  c.aux = &slot->aux;
  bptr const trace0 = slot->trace;
  bptr const ws0 = (bptr)(slot + 1);

  // mode 0: the run state is shared by all cases
  Rng parent; int gen0 = 0; uint32_t pri0 = 0, meta0 = 0; int nfs0 = 0;
  if (p.mode == 0) {
    const EH_G RunState* rs = p.run;
    parent.a1 = rs->a1; parent.a2 = rs->a2; parent.a3 = rs->a3; parent.draws = 0;
    gen0 = rs->gen; nfs0 = rs->nfs;
    if (l < nfs0) {
      uint32_t name = rs->fs_name[l];
      pri0 = rs->fs_pri[l];
      meta0 = em_pack(rs->fs_score[l], name, name, name == M_SNAND ? (uint32_t)rs->snand_mask : 3u);
    }
  }

  // where the wave slots' time goes (eh_result_occupancy): this workgroup's life, its cases, its stay for posted chunks - 100 MHz ticks
  const unsigned long long wg_t0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long case_ticks = 0, linger_ticks = 0;
  const uint64_t TICKET_BATCH = 4;                // cases claimed per atomic (one counter saturates at ~88 dequeues/us)
  uint64_t tk_next = 0, tk_end = 0;
  while (true) {
    if (tk_next == tk_end) {
      unsigned long long t = 0;
      if (l == 0) t = atomicAdd(&p.ctr->ticket, (unsigned long long)TICKET_BATCH);
      tk_next = uni64(t); tk_end = tk_next + TICKET_BATCH;
    }
    if (p.board && uni(co_ld32(&p.board->open)) != 0) co_help(p.board, 2);   // chunks of heavy cases' loops, between two cases of my own
    uint64_t i = tk_next++;
    if (i >= p.n) {
#ifndef HIPEMU
      // Out of tickets: the pass ends with its heaviest cases, each on ONE wavefront, and what those post would find nobody between
      // two cases any more.  Up to CO_LINGER wavefronts of the pass stay for chunks - of any pass's cases - while the pass has
      // cases under way and some case on the device is posting; the others leave their slots to the workgroups of the next passes.
      if (p.board) {
        unsigned int mine = p.co_linger;
        if (l == 0) mine = (unsigned int)atomicAdd(&p.ctr->lingering, 1ull);
        if (uni(mine) < p.co_linger) {
          const unsigned long long lg0 = __builtin_amdgcn_s_memrealtime();
          EH_G CoBoard* bd = p.board;
          for (uint32_t spins = 0; spins < (1u << 24); spins++) {
            if (uni64(co_ld64(&p.ctr->done)) >= p.n || uni(co_ld32(&bd->posters)) == 0) break;
            if (uni(co_ld32(&bd->open)) != 0) co_help(bd, 8);
            else { for (int z = 0; z < 6; z++) __builtin_amdgcn_s_sleep(127); }   // ~20 us: posted loops last hundreds (every poll is a trip to the L2 of all these wavefronts)
          }
          linger_ticks = __builtin_amdgcn_s_memrealtime() - lg0;
        }
      }
#endif
      break;
    }
    c.co_posted = 0;
    const unsigned long long case_t0 = __builtin_amdgcn_s_memrealtime();
    uint64_t tick0 = __builtin_readcyclecounter();
#ifndef HIPEMU
    c.t_case = tick0;
#else
    c.t_case = 0;                                                          // the emulator's lanes read their own clocks
#endif
    c.nchunk = 0; c.ws_peak = 0; c.ws_top = 0;
    c.trace = (p.flags & EH_FLAG_META_TRACE) ? trace0 : nullptr; c.ntrace = 0; c.tr_base = 0; c.m_aux = -1;
    c.ch_vstart[0] = 0; c.ch_vend[0] = p.work_cap; c.ch_base[0] = ws0; c.ch_tier[0] = 0; c.ch_area[0] = slot_id;
    ws_set_view(c, 0);
    for (int d = 0; d < LEX_LEVELS; d++) c.lex_ptr[d] = 0;
    unsigned long long base = 0; uint64_t total = 0;
    c.work = 0; c.depth = 0;
    c.status = CASE_OK; c.lastm = -1; c.nb = 0; c.cur = 0; c.nem = 0; c.ws_used = 0;
    c.r_kind = R_SAME; c.r_flush = 0; c.r_drop_next = 0; c.r2 = 0;
    if (l == 0) { c.aux->nest.st[0].count = 0; c.aux->nest.st[1].count = 0; for (int d = 0; d < LEX_LEVELS; d++) { EH_G LexCache& lc = c.aux->lex[d]; lc.n = -1; lc.tcap = 0; } c.aux->nest.fo.has = 0; }
    wave_sync();
    int gen;
    Rng pr;
    c.max_block_scaled = p.cfg.max_block_scaled; c.min_block_scaled = p.cfg.min_block_scaled;
    if (p.mode == 0) {
      // ThreadSeed of case I = parent draws 3(I-1)+1..3(I-1)+3   (erlamsa_main.erl:179, erlamsa_rnd.erl:65)
      pr = parent;
      rng_skip(pr, 3 * (p.first_case + i - 1));
      gen = gen0; lt.e_pri = pri0; lt.e_meta = meta0; c.nfs = nfs0;
    } else {
      int mask;
      SelView sel = {p.cfg.nsel, p.cfg.sel_name, p.cfg.sel_pri};
      if (p.profile_id) {
        const EH_G ProfileCfg* pf = p.profiles + uni(p.profile_id[i]);     // the case's option profile, wave-uniform (the host has checked every id against the table's size)
        c.max_block_scaled = uni(pf->max_block_scaled); c.min_block_scaled = uni(pf->min_block_scaled);
        sel.nsel = (int32_t)uni((uint32_t)pf->nsel); sel.sel_name = pf->sel_name; sel.sel_pri = pf->sel_pri;
      }
      setup_run(sel, p.cfg, p.seeds[3 * i], p.seeds[3 * i + 1], p.seeds[3 * i + 2], pr, gen, mask, lt.e_pri, lt.e_meta, c.nfs);
    }
#ifdef EH_PROF
#define EH_PH(k) do { uint64_t now_ = __builtin_readcyclecounter(); if (l == 0) { atomicAdd(&p.prof[2 * (PROF_PHASE + (k))], (unsigned long long)(now_ - ph0)); atomicAdd(&p.prof[2 * (PROF_PHASE + (k)) + 1], 1ull); } ph0 = now_; } while (0)
    uint64_t ph0 = __builtin_readcyclecounter();
#else
#define EH_PH(k) do {} while (0)
#endif
    int64_t t1 = (int64_t)rng_erand(pr, 99999), t2 = (int64_t)rng_erand(pr, 99999), t3 = (int64_t)rng_erand(pr, 99999);
    c.rng.draws = 0;
    rng_seed(c.rng, t1, t2, t3);                                        // worker: erlamsa_rnd:seed(ThreadSeed) :183

    uint64_t o0 = p.coff[p.corpus_first + i], o1 = p.coff[p.corpus_first + i + 1];
    o0 = uni64(o0); o1 = uni64(o1);
    EH_PH(0);
    c.gen_pending = 0;                                                                               // DataGen() :185
    if (gen == G_DIRECT) gen_direct(c, p.corpus + o0, (uint32_t)(o1 - o0));
    else if (gen == G_RANDOM) gen_random(c);
    else if (gen == G_FILE) { c.gen_e1 = rng_erand(c.rng, (uint32_t)p.n_paths) - 1; c.gen_pending = G_FILE; }          // file_streamer :108-110
    else { c.gen_e1 = rng_erand(c.rng, (uint32_t)p.n_paths) - 1; c.gen_e2 = rng_erand(c.rng, (uint32_t)p.n_paths) - 1; c.gen_pending = G_JUMP; }   // jump_streamer :138
    EH_PH(1);

    if (c.status == CASE_OK) {
      // choose_pattern_fun (erlamsa_patterns.erl:431-434) + choose_pri
      const int pat = p.mode != 0 && p.profile_id ? choose_pattern(p.profiles[uni(p.profile_id[i])], c.rng) : choose_pattern(p.cfg, c.rng);
      if (pat < 0) c.status = CASE_CRASHED; else run_patterns(c, lt, pat);  // Pat(Ll, CurMuta, Meta) :189
    }

    EH_PH(2);
    // ---- erlamsa_out:output/4: concatenate the written blocks into the output arena
    wave_sync();                                                        // (the last pieces were written by lane 0 just now)
    total = 0; base = 0;
    if (c.status == CASE_OK) for (int k = 0; k < c.nem; k++) total += blk_load(c.em, k).len;
    if (total > 0) {
      if (l == 0) base = atomicAdd(p.out_cursor, (unsigned long long)((total + 15) & ~15ull));
      base = uni64(base);
      if (base + total > p.out_cap) { c.status = CASE_ARENA_FULL; total = 0; }
    }
    if (total > 0) {
      uint64_t pos = base;
      for (int k = 0; k < c.nem; k++) { Blk b = blk_load(c.em, k); wave_copy(p.out + pos, (cbptr)b.ptr, b.len); pos += b.len; }
    }
    // the case's meta trace goes behind its output in the arena
    unsigned long long tbase = 0;
    if (c.trace && c.ntrace > 0) {
      wave_sync();
      if (l == 0) tbase = atomicAdd(p.out_cursor, (unsigned long long)((c.ntrace + 15u) & ~15u));
      tbase = uni64(tbase);
      if (tbase + c.ntrace > p.out_cap) { c.ntrace = 0; if (c.status == CASE_OK) { c.status = CASE_ARENA_FULL; total = 0; } }
      else wave_copy(p.out + tbase, c.trace, c.ntrace);
    }
    EH_PH(3);
#ifndef HIPEMU
    __builtin_amdgcn_s_setprio(0);                                      // (mux_fuzzers raises it for cases that run long)
#endif
    if (c.co_posted && l == 0) atomicAdd(&p.board->posters, 0xFFFFFFFFu);   // (- 1)
    if (l == 0) {
      atomicAdd(&p.ctr->done, 1ull);                                      // cases of the pass that are done (the lingering wavefronts watch it)
      atomicAdd(&p.ctr->out_bytes, (unsigned long long)total);                  // the batch's totals on the device (eh_result_summary: one small copy instead of n lengths and n statuses)
      atomicAdd(&p.ctr->by_status[c.status >= 0 && c.status < 6 ? c.status : 1], 1ull);
    }
    // larger areas the case borrowed go back to the pool (the output has been copied out of them)
    wave_sync();
    if (c.nchunk > 0) ws_release_to(c, 0);
    if (l == 0) {
      p.out_off[i] = base; p.out_len[i] = total; p.status[i] = c.status;
      p.draws[i] = c.rng.draws; p.lastm[i] = c.status == CASE_OVERFLOW ? -c.ovf_line : c.lastm; p.cycles[i] = __builtin_readcyclecounter() - tick0;
      p.peak[i] = c.ws_peak + c.ws_top;
      if (p.flags & EH_FLAG_META_TRACE) { p.trace_off[i] = tbase; p.trace_len[i] = c.trace ? c.ntrace : 0u; }
    }
    case_ticks += __builtin_amdgcn_s_memrealtime() - case_t0;
    wave_sync();
  }
  // The last workgroup to leave writes the batch's totals into page-locked host memory: a host loop over many batches then needs no
  // copy call per batch (a hipMemcpy of a few bytes from a device full of persistent workgroups took the bench's host thread 60 - 90
  // ms per step, during which it launched nothing).  Every wavefront's counter updates are complete before its own increment
  // returns (the returned value is waited for with vmcnt(0)), so the one that sees all the others reads final values.
  wave_sync();
  unsigned long long left = 0;
  if (l == 0) {
    atomicAdd(&p.ctr->wg_ticks, __builtin_amdgcn_s_memrealtime() - wg_t0);
    atomicAdd(&p.ctr->case_ticks, case_ticks);
    atomicAdd(&p.ctr->linger_ticks, linger_ticks);
  }
  if (l == 0) left = atomicAdd(&p.ctr->left, 1ull);
  if (uni64(left) + 1 == (unsigned long long)gridDim.x && p.summary_out) {
    if (l < 6) sys_store(&p.summary_out->by_status[l], co_ld64(&p.ctr->by_status[l]));
    if (l == 6) { sys_store(&p.summary_out->out_bytes, co_ld64(&p.ctr->out_bytes)); sys_store(&p.summary_out->n, p.n); }
    if (l == 7) { sys_store(&p.summary_out->wg_ticks, co_ld64(&p.ctr->wg_ticks)); sys_store(&p.summary_out->case_ticks, co_ld64(&p.ctr->case_ticks)); sys_store(&p.summary_out->linger_ticks, co_ld64(&p.ctr->linger_ticks)); sys_store(&p.summary_out->workgroups, (unsigned long long)gridDim.x); }
    wave_sync();
    if (l == 0) sys_store(&p.summary_out->seq, p.batch_seq);
  }
}

// =============================================================================================
// EH_FLAG_ORDERED_OUTPUT: compaction of the completion-ordered arena into case order
// =============================================================================================
// ord_off[i] = sum of out_len[0..i): one wavefront, 64 cases per step (n / 64 shuffle scans)
__global__ void __launch_bounds__(64) eh_order_scan_kernel(const uint64_t* out_len_, uint64_t* ord_off_, uint64_t n) {
  cqptr out_len = (cqptr)out_len_; qptr ord_off = (qptr)ord_off_;
  const int l = EH_LANE;
  uint64_t run = 0;
  for (uint64_t base = 0; base < n; base += 64) {
    uint64_t i = base + (uint64_t)l;
    uint64_t v = i < n ? out_len[i] : 0;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      uint64_t t = ((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(inc >> 32), d) << 32) | (uint32_t)__shfl_up((int)(uint32_t)inc, d);
      if (l >= d) inc += t;
    }
    if (i < n) ord_off[i] = run + inc - v;
    run += uni64(((uint64_t)(uint32_t)__shfl((int)(uint32_t)(inc >> 32), 63) << 32) | (uint32_t)__shfl((int)(uint32_t)inc, 63));
  }
  if (l == 0) ord_off[n] = run;
}
// one wavefront per case (grid-stride): dst[ord_off[i] ..) = src[out_off[i] ..)
__global__ void __launch_bounds__(64) eh_order_gather_kernel(const uint8_t* src_, uint8_t* dst_, const uint64_t* out_off_, const uint64_t* out_len_,
                                                             const uint64_t* ord_off_, uint64_t n, uint64_t ord_base) {
  cbptr src = (cbptr)src_; bptr dst = (bptr)dst_; cqptr out_off = (cqptr)out_off_, out_len = (cqptr)out_len_, ord_off = (cqptr)ord_off_;
  for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
    uint64_t len = uni64(out_len[i]), so = uni64(out_off[i]), d0 = uni64(ord_off[i]) - ord_base;
    uint64_t done = 0;
    while (done < len) { uint32_t c = len - done > 0x40000000ull ? 0x40000000u : (uint32_t)(len - done); wave_copy_raw(dst + d0 + done, src + so + done, c); done += c; }
  }
}

__global__ void __launch_bounds__(64) eh_test_copy_kernel(uint8_t* buf_, const uint32_t* jobs_, uint32_t njobs, uint32_t* eq_out_) {
  bptr buf = (bptr)buf_; cwptr jobs = (cwptr)jobs_; wptr eq_out = (wptr)eq_out_;
  g_ctx.p = nullptr;                                             // (not a case: nothing is posted for other wavefronts, co_run)
  // job = {kind, dst_off, src_off, n, plen}: kind 0 copy, 1 periodic fill, 2 equal
  for (uint32_t j = blockIdx.x; j < njobs; j += gridDim.x) {
    uint32_t kind = jobs[5 * j], d = jobs[5 * j + 1], s = jobs[5 * j + 2], n = jobs[5 * j + 3], pl = jobs[5 * j + 4];
    if (kind == 0) wave_copy_raw(buf + d, buf + s, n);
    else if (kind == 1) wave_fill_periodic(buf + d, buf + s, pl, n);
    else if (kind == 2) { bool e = wave_equal_raw(buf + d, buf + s, n); if (EH_LANE == 0) eq_out[j] = e ? 1u : 0u; }
    else {  // kind 3: mask window self check over buf[s, s+n) with window base d (multiple of 64)
      MaskWin<4> a, b; a.p = buf + s; a.L = n; b.p = buf + s; b.L = n;
      mw_load(a, d, LexCls()); mw_load_ref(b, d, LexCls());
      uint32_t bad = 0;
      for (int k = 0; k < 4; k++) bad += a.m[k] != b.m[k] ? 1u : 0u;
      bad += a.inrange != b.inrange ? 1u : 0u;
      MaskWin<4> c2, d2; c2.p = buf + s; c2.L = n; d2.p = buf + s; d2.L = n;
      mw_load(c2, d, DelimCls()); mw_load_ref(d2, d, DelimCls());
      for (int k = 0; k < 4; k++) bad += c2.m[k] != d2.m[k] ? 1u : 0u;
      bad = wave_sum(bad);
      if (EH_LANE == 0) eq_out[j] = bad;
    }
    wave_sync();
  }
}

// Self test of eh_zlib.h: op 0..2 compress in[0..n) as ZF_RAW / ZF_GZIP / ZF_ZLIB, op 4 / 5 = zlib:gunzip / zlib:inflate semantics
// (z_uncompress_size + z_uncompress_write); res[0] = bytes written, res[1] = 1 ok / 0 "raises".
__global__ void __launch_bounds__(64) eh_test_zlib_kernel(int op, const uint8_t* in_, uint64_t n, uint8_t* out_, uint64_t cap, uint8_t* scratch_, uint64_t* res_) {
  cbptr in = (cbptr)in_; bptr out = (bptr)out_, scratch = (bptr)scratch_; qptr res = (qptr)res_;
  g_ctx.p = nullptr;
  uint64_t len = 0; int ok = 1;
  if (op <= 2) { len = z_compress((EH_G ZDef*)scratch, op, in, n, out, cap); ok = len != 0; }
  else {
    EH_G ZInf* zi = (EH_G ZInf*)scratch; uint64_t off = 0;
    ok = z_uncompress_size(zi, op - 3, in, n, &len, &off);
    if (ok && len > cap) ok = 0;
    if (ok) ok = z_uncompress_write(zi, op - 3, in, n, off, out, len);
  }
  if (EH_LANE == 0) { res[0] = len; res[1] = (uint64_t)ok; }
}

}  // namespace eh

// Batches in flight on several HIP streams (one context each) only run side by side when every stream gets a hardware queue of its
// own; the runtime maps streams onto GPU_MAX_HW_QUEUES of them (default 4: with six passes in flight pairs of them serialise,
// 21.7 instead of 33.7 GB/s, profiles/r04_bench_q4.json).  The variable is read when the HIP runtime initialises, i.e. at the first
// HIP call of the process: set here, when the library is loaded, unless the host has asked for eight or more itself.  (A process that
// has used HIP before it loads this library - a torch that came first - keeps what it started with: INTEGRATION.md section 3.)
#include "eh_host_queues.h"
__attribute__((constructor)) static void eh_runtime_defaults() {
  // The rule is hw_queues_to_write (eh_host_queues.h): eight when the variable is not set or is a plain decimal number below eight -
  // a 4 in the environment is the runtime's default written out by whoever started the process, and puts seven streams on four
  // queues -, nothing otherwise: never lowered, nothing above eight, and what is no number is left to the runtime.  Once, and only
  // here - at load time, before this library has made a HIP call.  A host that loads the library into a process with threads already
  // running (a BEAM: setenv is not safe against a concurrent getenv) exports GPU_MAX_HW_QUEUES=8 itself before it starts, and a
  // process where torch initialised HIP first exports it before torch does; both still see no setenv here (INTEGRATION.md section 3,
  // note 0).
  const int want = eh::hw_queues_to_write(getenv("GPU_MAX_HW_QUEUES"));
  if (want) { char v[16]; snprintf(v, sizeof v, "%d", want); setenv("GPU_MAX_HW_QUEUES", v, 1); }
}

// =============================================================================================
// host side: one header per subject, in an order that needs no forward declaration
// =============================================================================================
#include "eh_host.h"
#include "eh_host_pool.h"
#include "eh_host_launch.h"
#include "eh_host_corpus.h"
#include "eh_host_results.h"
#include "eh_host_coalesce.h"
#include "eh_host_options.h"
#include "eh_host_unique.h"
#include "eh_host_seen.h"
#include "eh_host_promote.h"
#include "eh_host_selftest.h"
