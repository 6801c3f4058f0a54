// eh_common.h — ids, tables and plain structs shared by the host API and the
// device kernels of liberlamsa_hip.so.
#pragma once
#include <stddef.h>
#include <stdint.h>

// Everything the kernels read and write besides their registers, the LDS and their stack is HBM (corpus arena, slots, pool areas,
// output arena, result arrays).  Device code says so in the pointer TYPE: address space 1, so loads and stores are global_*
// instructions.  A generic pointer makes them flat_*: an aperture check per access, and - what costs - a flat access counts in
// vmcnt AND lgkmcnt, so every LDS read of the per-case context (g_ctx) waits for the HBM traffic in flight.  Global converts to
// generic implicitly, never the other way round: a pointer into the LDS or the stack cannot end up in one of these types unseen.
// The host pass and the CPU emulator (tests/hipemu) see plain pointers.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(HIPEMU)
#define EH_G __attribute__((address_space(1)))
#else
#define EH_G
#endif

namespace eh {

typedef EH_G uint8_t* bptr;   typedef const EH_G uint8_t* cbptr;
typedef EH_G uint32_t* wptr;  typedef const EH_G uint32_t* cwptr;
typedef EH_G uint64_t* qptr;  typedef const EH_G uint64_t* cqptr;

// Mutator ids in the table order of erlamsa_mutations:mutations/1
// (reference src/erlamsa_mutations.erl:1291-1331).
enum MutaId : int {
  M_SGM, M_JS, M_UW, M_UI, M_AB, M_AD, M_TR2, M_TD, M_NUM, M_TS1, M_TR, M_TS2, M_BD, M_BEI, M_BED,
  M_BF, M_BI, M_BER, M_BR, M_SP, M_SR, M_SD, M_SNAND, M_SRND, M_LD, M_LDS, M_LR2, M_LRI, M_LR,
  M_LS, M_LP, M_LIS, M_LRS, M_FT, M_FN, M_FO, M_LEN, M_B64, M_URI, M_ZIP, M_NIL, M_COUNT
};
// Pattern ids in the table order of erlamsa_patterns:patterns/0 (erlamsa_patterns.erl:395-405).
enum PatId : int { P_OD, P_ND, P_BU, P_SK, P_SZ, P_CS, P_AR, P_CP, P_CO, P_NU, P_COUNT };
enum GenId : int { G_DIRECT = 0, G_RANDOM = 1, G_FILE = 2, G_JUMP = 3, G_COUNT = 4 };   // erlamsa_gen:generators/0 (stdin, genfuz: host I/O, not here)

enum CaseStatus : int { CASE_OK = 0, CASE_CRASHED = 1, CASE_OVERFLOW = 2, CASE_UNSUPPORTED = 3, CASE_ARENA_FULL = 4, CASE_BUDGET = 5 };

constexpr int MAX_FS = 64;          // mux_fuzzers list entries (one per lane of the wavefront)
constexpr int MAX_BLOCKS = 2048;    // block-list entries per case
constexpr int MAX_EMITS = 4096;     // deferred output pieces per case
constexpr int MAX_FRAMES = 16;      // nested sizer/csum wrappers
constexpr uint32_t TRACE_CAP = 32768; // meta-trace bytes kept per case (EH_FLAG_META_TRACE); the last byte is 0xFF when events were dropped

// ---- meta trace (ABI 7): the reference's Meta list of a case, element by element, in the order erlamsa_main.erl:58-70 prints it
// (lists:reverse(lists:flatten(Meta)), every element with ~p on a line of its own).  An event is a kind byte and its operands;
// atoms are ids into the table below (the 41 mutator codes first, in MutaId order), integers are LEB128 varints (zigzag where
// they can be negative).  eh_result_meta hands the bytes over as they are; eh_meta_atom_name names the atoms; the renderers are
// erlamsa_amd/meta.py and erlang/src/erlamsa_hip.erl meta_terms/1.
enum TraceKind : int {
  TRK_AA = 1,       // {Atom, Atom}            [a][b]                         {failed, sgm} {pattern, once_dec} {compressed, gzip}
  TRK_AI = 2,       // {Atom, Integer}         [a][zigzag varint]             {byte_drop, -1} {seq_repeat, 4096} {skipped_big, N}
  TRK_SIZER = 3,    // {sizer, {ok, Size, big | little, Len, A, B}}  [Size/8][big][varint Len][varint A][varint B]   erlamsa_patterns.erl:97
  TRK_CSUM = 4,     // {csum, {xor8 | crc32, Size, PLen, BLen}}      [crc][varint PLen][varint BLen]                  :131
  TRK_SKIPPED = 5,  // {skipped, Len/8}        [varint bytes]                 the float of a whole number :154
  TRK_ARCHIVER = 6, // {archiver, Name}        [varint n][n bytes]            the file name :183
};
#define EH_ATOMS(X)                                                                                                              \
  X(sgm) X(js) X(uw) X(ui) X(ab) X(ad) X(tr2) X(td) X(num) X(ts1) X(tr) X(ts2) X(bd) X(bei) X(bed) X(bf) X(bi) X(ber) X(br) X(sp)  \
  X(sr) X(sd) X(snand) X(srnd) X(ld) X(lds) X(lr2) X(lri) X(lr) X(ls) X(lp) X(lis) X(lrs) X(ft) X(fn) X(fo) X(len) X(b64) X(uri)  \
  X(zip) X(nil)                                                                                                                   \
  X(failed) X(used) X(pattern) X(skipped_big) X(once_dec) X(many_dec) X(burst) X(skipper) X(sizer) X(csum) X(archiver)            \
  X(compressed) X(no_muta) X(mutate_once) X(empty_stopped) X(decompressed) X(gzip) X(zlib) X(ok) X(success) X(json)               \
  X(base64_mutator) X(sed_utf8_widen) X(sed_utf8_insert) X(ascii_bad) X(ascii_delimeter) X(tree_dup) X(tree_del) X(muta_num)      \
  X(tree_swap_one) X(tree_stutter) X(tree_swap_two) X(byte_drop) X(byte_inc) X(byte_dec) X(byte_flip) X(byte_insert)              \
  X(byte_swap_random) X(byte_repeat) X(seq_perm) X(seq_repeat) X(seq_drop) X(seq_randmask) X(line_del) X(line_del_seq)            \
  X(line_dup) X(line_clone) X(line_repeat) X(line_swap) X(line_perm) X(list_ins) X(list_replace) X(fuse_this) X(fuse_next)        \
  X(fuse_old) X(muta_len) X(muta_zippath) X(nomutation) X(json_swap) X(json_dup) X(json_pump) X(json_repeat) X(json_insert)       \
  X(json_unserialize) X(json_innertext) X(null) X(bool) X(sgml_swap) X(sgml_dup) X(sgml_pump) X(sgml_repeat) X(sgml_insert2)      \
  X(sgml_permparams) X(sgml_breaktag) X(sgml_insert) X(sgml_xmlfeatures) X(xmlns) X(sgml_innertext)
enum AtomId : int {
#define EH_ATOM_ENUM(n) AT_##n,
  EH_ATOMS(EH_ATOM_ENUM)
#undef EH_ATOM_ENUM
  AT_COUNT
};
static_assert((int)AT_nil == (int)M_NIL && (int)AT_sgm == (int)M_SGM && (int)AT_b64 == (int)M_B64, "the mutator codes are the first atoms, in MutaId order");
constexpr int POOL_TIERS = 8;       // tiers of larger work areas a case can borrow from

// erlamsa.hrl:44-58
constexpr uint32_t INITIAL_IP = 24;
constexpr uint32_t AVG_BLOCK_SIZE = 2048;
constexpr uint32_t MIN_BLOCK_SIZE = 256;
constexpr uint32_t MAX_BLOCK_SIZE = 4096;
constexpr uint32_t ABSMAXHALF_BINARY_BLOCK = 500000;
constexpr uint32_t ABSMAX_BINARY_BLOCK = 1000000;
constexpr uint32_t SIZER_MAX_FIRST_BYTES = 512;
constexpr uint32_t PREAMBLE_MAX_BYTES = 32;

// A block (binary) of the case's lazy list: generic pointer + length.
struct Blk {
  uint64_t ptr;
  uint32_t len;
  uint32_t aux;
};

// Result of the per-run setup of erlamsa_main:fuzzer/1 (:134-158): parent PRNG state after the
// setup draws, generator choice, and the initial mux_fuzzers list in list order.
struct RunState {
  uint32_t a1, a2, a3;       // parent stream state after setup (next draws = ThreadSeeds)
  int32_t gen;               // GenId
  int32_t nfs;
  int32_t snand_mask;        // 0 nand, 1 or, 2 xor
  uint8_t fs_name[MAX_FS];   // MutaId per list position
  uint8_t fs_score[MAX_FS];
  uint32_t fs_pri[MAX_FS];
};

struct DevConfig {
  // selected mutators in TABLE order (make_mutator folds over the table): name id, pri
  int32_t nsel;
  uint8_t sel_name[MAX_FS];
  uint32_t sel_pri[MAX_FS];
  // patterns after erlamsa_utils:sort_by_priority (erlamsa_utils.erl:113-117)
  int32_t npat;
  int32_t pat_total;
  uint8_t pat_id[P_COUNT];
  uint32_t pat_pri[P_COUNT];
  // generators after sort_by_priority
  int32_t ngen;
  int32_t gen_total;
  uint8_t gen_id[G_COUNT];
  uint32_t gen_pri[G_COUNT];
  uint32_t max_block_scaled;  // round(MAX_BLOCK_SIZE * blockscale)
  uint32_t min_block_scaled;  // round(MIN_BLOCK_SIZE * blockscale)
  // SSRF endpoint strings pre-rendered on the host
  char ssrf_host[64];
  char ssrf_port[12];
};

// ---- option profiles (eh_profile_add): what erlamsa_esi:parse_headers/2 reads from EVERY request besides the seed
// (erlamsa_esi.erl:30-68) - mutations, patterns, blockscale - as the fields of DevConfig a case takes from its profile instead of from
// the context's configuration.  Generators, the SSRF endpoint and every limit stay the context's (KParams::cfg).
constexpr uint32_t MAX_PROFILES = 1024;   // EH_MAX_PROFILES
struct ProfileCfg {
  int32_t nsel;                      // as DevConfig, field by field
  uint8_t sel_name[MAX_FS];
  uint32_t sel_pri[MAX_FS];
  int32_t npat;
  int32_t pat_total;
  uint8_t pat_id[P_COUNT];
  uint8_t pad[2];
  uint32_t pat_pri[P_COUNT];
  uint32_t max_block_scaled;
  uint32_t min_block_scaled;
};

// ---- cooperative execution of a heavy case's bulk loops (eh_device.h co_run / co_help) -------------------
// A case runs on ONE wavefront.  Loops over hundreds of kilobytes - block copies, the final concatenation, the streaming
// passes of eh_fuse2.h - are cut into chunks and posted on a board all contexts of the device share; wavefronts that are
// BETWEEN cases take chunks before they draw their next ticket, the poster takes chunks too and waits for the rest.
// word[j] = generation << 32 | chunks handed out (odd generation: open); a chunk is claimed by ONE atomic add, so its number and
// the job it belongs to are read together.
constexpr uint32_t CO_JOBS = 64, CO_ARGS = 12;
enum CoKind : uint32_t { CO_COPY = 1, CO_EQUAL = 2, CO_FBPASS = 3, CO_FBCOUNT = 4 };
struct CoJob {
  uint64_t a[CO_ARGS];          // arguments of the loop (kind-specific)
  unsigned long long acc;       // what the chunks add up to (members alive, mismatches found ...)
  uint32_t kind, nchunks, done, pad;
};
// indices of CoBoard::stat, in the order eh_coop_stats documents (ABI)
enum CoStat : int {
  CO_ST_POSTED = 0,        // jobs posted
  CO_ST_BY_HELPERS = 1,    // chunks run by helpers ...
  CO_ST_BY_POSTERS = 2,    // ... and by the posters themselves
  CO_ST_POSTER_WAIT = 3,   // cycles posters waited for the last chunks
  CO_ST_BOARD_FULL = 4,    // jobs that found no free entry
  CO_ST_COUNT = 8,         // words eh_coop_stats hands out (the rest: zero)
};
struct CoBoard {
  unsigned long long word[CO_JOBS];
  uint32_t owner[CO_JOBS];      // 1: a poster holds the entry
  uint32_t open;                // entries with chunks to hand out
  uint32_t posters;             // cases under way that have posted a loop: wavefronts whose pass has run out of tickets stay for chunks while there are any
  uint32_t pad[14];
  unsigned long long stat[CO_ST_COUNT];
  CoJob job[CO_JOBS];
};

// ---- memory the kernels and the host ABI both address by position.  The numbers in the static_asserts are the layout: bench.py, tools/
// and the callers of eh_result_prof / eh_pool_stats read by word number, so no member may move.
// EH_PROF slots: BatchCounters::prof[2 * k] and [2 * k + 1] - cycles and calls, or two counts: see the site.  Slots 0 .. M_COUNT - 1 are
// the mutators' (mux_fuzzers, by MutaId).  The values are what bench.py and tools/ read by number.  Slots with two users, as they stand:
// 85 and 86 (tree and sgm), 100 .. 103 (the two fuse searches: a call takes one or the other), 112 .. 120 (sgm, and fuse's calls by size).
enum ProfSlot : int {
  PROF_B64_LEX = 48,         // b64: lexing, candidates refused, decode, nested call, encode, gather
  PROF_B64_REFUSED = 49,
  PROF_B64_DECODE = 50,
  PROF_B64_NESTED = 51,
  PROF_B64_ENCODE = 52,
  PROF_B64_GATHER = 53,
  PROF_FR_SEARCH = 54,       // fuse on shortened lists (eh_fuse_red.h): the search
  PROF_FR_MEMBERS = 55,      // ... the node's members found in the original lists
  PROF_WS_FAILED = 56,       // work memory taken by attempts that failed (mux_fuzzers)
  PROF_WS_CAND = 57,         // ... the candidates that were used
  PROF_WS_BESIDES = 58,      // ... what the used attempts took besides their candidate
  PROF_PAT_PICK_CSUM = 59,   // patterns: pick_csum
  PROF_PAT_PICK_LEN = 60,    // pick_simple_len
  PROF_PAT_CS_BLOB = 61,     // cs: the checksummed bytes gathered
  PROF_PAT_CS_SUM = 62,      // cs: the checksum
  PROF_PAT_CP_BEGIN = 63,    // cp: pat_container_begin (ar: 78)
  PROF_PHASE = 64,           // + k: the phases of a case in eh_mutate_kernel (EH_PH(0 .. 3))
  PROF_SG_BATCH_FAILED = 68, // sgm: failed attempts committed by lane batches
  PROF_PAT_CP_END = 69,      // cp: the wrapper popped (ar: 79)
  PROF_TREE = 70,            // + k: eh_tree.h TR_PH / TR_ST, k = 0 .. 7 and 10 .. 15
  PROF_PAT_AR_BEGIN = 78,
  PROF_PAT_AR_END = 79,
  PROF_SG_BATCH_TAGS = 85,   // sgm: tags written by lane batches, batches           (also PROF_TREE + 15: events, parses)
  PROF_TREE_LANES = 86,      // tree: events decided by lane batches, quotes
  PROF_SG_TEXT = 86,         // sgm tokenizer: text state + bookkeeping between attempts
  PROF_SG_TAG_FAILED = 87,   // ... failed attempts
  PROF_SG_TAG_OK = 88,       // ... accepted tags
  PROF_SG_PERIOD_LOST = 89,  // sgm replay: gave up, never back in the state a period later
  PROF_SG_TOKENIZE = 90,     // sgm: sgml_tokenize, sgml_flags, the mutation, the result gathered
  PROF_SG_FLAGS = 91,
  PROF_SG_MUTATE = 92,
  PROF_SG_GATHER = 93,
  PROF_SG_REPLAY = 94,       // sgm replay: tokens written, replays
  PROF_SG_STRETCH = 95,      // sgm: stretches found, searches
  PROF_FB_PASS_N1_LDS = 96,  // fuse, streaming search (eh_fuse2.h): a pass by where its tables are - also 105 .. 107, 110, 111
  PROF_FR_CUTS = 97,         // fuse on shortened lists: finding + making the cuts, calls that took them
  PROF_FR_NO_CUT = 98,       // ... calls that found none
  PROF_SG_NO_REPLAY = 99,    // sgm: checked but not replayed; of them: look-ahead too long
  PROF_FB_ALLOC = 100,       // fuse, streaming search: a round's steps
  PROF_FB_BITS0 = 101,
  PROF_FB_ETEST = 102,
  PROF_FB_SCAN = 103,
  PROF_FL_ROUND1 = 100,      // fuse, search in LDS (eh_fuse_lds.h): first round, later rounds, rounds of single members, the choice
  PROF_FL_ROUNDS = 101,
  PROF_FL_SINGLE = 102,
  PROF_FL_SELECT = 103,
  PROF_FB_CLEAR = 104,
  PROF_FB_PASS_LDS = 105,
  PROF_FB_PASS_GLOBAL = 106,
  PROF_FB_PASS_LAST = 107,
  PROF_FB_TAIL = 108,
  PROF_FB_SELECT = 109,
  PROF_FB_PASS_TEST = 110,
  PROF_FB_PASS_N1 = 111,
  PROF_FUSE_BY_SIZE = 112,   // + b: fuse calls by log2(la + lb), b = 0 .. 13
  PROF_SG_SETUP = 112,       // sgm tokenizer: set-up, after an accepted tag, lane batches, the next '<'
  PROF_SG_AFTER_ACCEPT = 113,
  PROF_SG_LANE_BATCHES = 114,
  PROF_SG_FIND_LT = 115,
  PROF_SG_NEXT_STOP = 116,   // sgm: building the next-stop table
  PROF_SG_PHASE1 = 117,      // sgm: the tokenizer's first phase
  PROF_SG_ATTRS_WALKED = 118,// sgm: attributes an attempt walked
  PROF_SG_EVENTS = 119,      // sgm: events found, bytes tokenized
  PROF_SG_ATTRS = 120,       // sgm: attributes written by attribute batches, batches
  PROF_FUSE_ROUNDS = 126,    // fuse: refinement rounds, calls
  PROF_WG_START = 127,       // earliest / latest workgroup start of the dispatch (atomicMin / atomicMax, not sums)
  PROF_SLOTS = 128,
};

// The counters of a batch (Results::d_counters): zeroed by eh_prologue_kernel, added to by eh_mutate_kernel.
struct BatchCounters {
  unsigned long long ticket;        // next case to hand out
  unsigned long long out_cursor;    // bump cursor of the output arena (KParams::out_cursor)
  unsigned long long in_bytes;      // (KParams::in_bytes)
  unsigned long long done;          // cases of the pass that are done (the lingering wavefronts watch it)
  unsigned long long lingering;     // wavefronts that stayed for posted chunks
  unsigned long long out_bytes;     // output bytes of the batch
  unsigned long long left;          // workgroups that have left
  unsigned long long wg_ticks;      // 100 MHz ticks: the workgroups' lifetimes ...
  unsigned long long prof[2 * PROF_SLOTS];   // EH_PROF builds (KParams::prof, eh_result_prof)
  unsigned long long by_status[6];  // cases of the batch by CaseStatus
  unsigned long long pad0[2];
  unsigned long long case_ticks;    // ... their time in cases ...
  unsigned long long linger_ticks;  // ... and lingering for posted chunks
  unsigned long long pad1[238];
};
static_assert(sizeof(BatchCounters) == 4096, "BatchCounters: 512 words");
static_assert(offsetof(BatchCounters, ticket) == 0 && offsetof(BatchCounters, out_cursor) == 8 && offsetof(BatchCounters, in_bytes) == 16 &&
              offsetof(BatchCounters, done) == 24 && offsetof(BatchCounters, lingering) == 32 && offsetof(BatchCounters, out_bytes) == 40 &&
              offsetof(BatchCounters, left) == 48 && offsetof(BatchCounters, wg_ticks) == 56 && offsetof(BatchCounters, prof) == 8 * 8 &&
              offsetof(BatchCounters, by_status) == 264 * 8 && offsetof(BatchCounters, case_ticks) == 272 * 8 &&
              offsetof(BatchCounters, linger_ticks) == 273 * 8, "BatchCounters: word numbers");

// The totals of a batch in page-locked host memory (Results::h_sum): the last workgroup of eh_mutate_kernel to leave writes them, `seq`
// last; eh_result_summary and eh_result_occupancy read them without a copy call.
struct BatchSummary {
  unsigned long long unused0;
  unsigned long long out_bytes;
  unsigned long long n;
  unsigned long long by_status[6];
  unsigned long long seq;           // KParams::batch_seq of the batch the values belong to
  unsigned long long wg_ticks, case_ticks, linger_ticks, workgroups;   // eh_result_occupancy out[0 .. 3], in this order
  unsigned long long pad[2];
};
static_assert(sizeof(BatchSummary) == 128, "BatchSummary: 16 words");
static_assert(offsetof(BatchSummary, out_bytes) == 8 && offsetof(BatchSummary, n) == 16 && offsetof(BatchSummary, by_status) == 24 &&
              offsetof(BatchSummary, seq) == 72 && offsetof(BatchSummary, wg_ticks) == 80 && offsetof(BatchSummary, case_ticks) == 88 &&
              offsetof(BatchSummary, linger_ticks) == 96 && offsetof(BatchSummary, workgroups) == 104, "BatchSummary: word numbers");

// The counters of the work-area pool (DevPool::d_ctr, KParams::pool_ctr).  Every tier t is a ring of free area indices.  eh_pool_stats
// copies words [0, 40) out as they are.
struct PoolCounters {
  struct { unsigned long long pop, push; } ring[10];   // tickets handed to poppers / pushers of tier t (the device: pool_tickets, eh_device.h)
  unsigned long long wait_ticks[10];                    // ticks wavefronts waited for an area of tier t
  unsigned long long waits[10];                         // how many had to wait
  unsigned long long most_out[10];                      // the most areas of tier t wanted at the same time
  unsigned long long pad[14];
};
static_assert(POOL_TIERS + 1 <= 10, "PoolCounters has ten tiers' room");
static_assert(sizeof(PoolCounters) == 64 * 8, "PoolCounters: 64 words");
static_assert(offsetof(PoolCounters, ring) == 0 && sizeof(PoolCounters::ring[0]) == 16 && offsetof(PoolCounters, wait_ticks) == 20 * 8 &&
              offsetof(PoolCounters, waits) == 30 * 8 && offsetof(PoolCounters, most_out) == 40 * 8, "PoolCounters: word numbers");

struct KParams {
  cbptr corpus;
  cqptr coff;
  uint64_t corpus_first;
  uint64_t n_paths;           // entries of the whole corpus: the Paths of the file / jump generators
  uint64_t n;
  uint64_t first_case;        // 1-based case number of case 0 (mode 0)
  int32_t mode;               // 0 batch (one parent seed), 1 per-call seeds
  const EH_G RunState* run;        // mode 0
  const EH_G int64_t* seeds;       // mode 1: 3n
  DevConfig cfg;
  uint64_t work_cap;          // bytes of the linear work area of a tier-0 slot
  uint64_t work_budget;       // per-case byte budget (sum of block sizes handed to mutators)
  uint64_t fuse_stream_min;   // fuse/2 on la + lb >= this many bytes runs as the position-indexed refinement of eh_fuse2.h
  // outputs
  bptr out;
  uint64_t out_cap;
  EH_G unsigned long long* out_cursor;
  qptr out_off;
  qptr out_len;
  EH_G int32_t* status;
  qptr draws;
  EH_G int32_t* lastm;
  qptr cycles;           // per-case shader-clock ticks (diagnostic)
  qptr peak;             // per-case work-memory high-water mark in bytes (diagnostic)
  qptr trace_off;        // EH_FLAG_META_TRACE: where the case's trace sits in `out` ...
  wptr trace_len;        // ... and its length in bytes (TraceKind events, above)
  uint32_t flags;             // EH_FLAG_*
  EH_G unsigned long long* prof;   // EH_PROF builds: BatchCounters::prof - [2*k] cycles, [2*k+1] calls of slot k (ProfSlot)
  EH_G BatchCounters* ctr;          // the batch's counters (out_cursor, in_bytes and prof above point into the same block)
  EH_G unsigned long long* in_bytes;
  // Work areas.  Workgroup w of a batch owns slot w of the context (block tables + work_cap bytes of work area): a slot per
  // launched workgroup, so no wavefront ever waits for one.  A case that outgrows what it holds borrows a larger area from
  // a POOL all contexts of the device share (eh_host.h DevPool, eh_host_pool.h; tiers 1..ntiers, twice the area per tier up to
  // big_case_bytes) and goes on there; only the mutator attempt that ran out of memory is repeated (eh_device.h, ws_regrow).
  // Every tier is a ring of free area indices; its tickets and waits are counted in PoolCounters.
  bptr slot_base;
  uint64_t slot_stride;
  int32_t ntiers;                // tiers of the pool (1..ntiers)
  bptr pool_base[POOL_TIERS + 1];   // tier t: area k at pool_base[t] + k * pool_stride[t]
  uint64_t pool_stride[POOL_TIERS + 1];
  uint64_t pool_cap[POOL_TIERS + 1];    // work-area bytes of an area of tier t (pool_cap[0] == work_cap: the slot's own)
  uint32_t pool_cnt[POOL_TIERS + 1];
  wptr pool_ring[POOL_TIERS + 1];
  EH_G PoolCounters* pool_ctr;
  EH_G CoBoard* board;          // nullptr: every case does all its work itself (EH_FLAG_NO_COOP)
  EH_G BatchSummary* summary_out;  // page-locked HOST memory: the last workgroup to leave writes the batch's totals there (eh_result_summary reads them without a copy call)
  uint64_t batch_seq;           // ... stamped with this number
  uint32_t co_copy_min, co_copy_chunk;   // bytes: copies / compares of co_copy_min and more are posted in chunks of co_copy_chunk
  uint32_t co_fb_min, co_fb_chunk;       // positions: the same for the streaming passes of eh_fuse2.h (chunk: a multiple of 1024)
  uint32_t co_linger, pad_co;            // wavefronts of a pass that stay for posted chunks once the pass is out of tickets
  // mode 1 with option profiles (eh_fuzz_calls_profiled): case i runs under profiles[profile_id[i]].  Both nullptr otherwise.
  const EH_G ProfileCfg* profiles;
  const EH_G uint32_t* profile_id;       // n
};

struct MutaInfo { const char* name; int pri; int on_gpu; };
struct PatInfo { const char* name; int pri; int on_gpu; };

}  // namespace eh
