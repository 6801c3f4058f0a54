// eh_patterns.h - device: the emit list, the split of a block list and the patterns (erlamsa_patterns.erl).  A part of
// eh_engine.hip, included there once, inside namespace eh, behind eh_prologue_kernel.
#pragma once
// =============================================================================================
// device: emit list, split, patterns
// =============================================================================================
EH_DEV void emit_ref(Ctx& c, uint64_t ptr, uint32_t len) {
  if (len == 0) return;
  if (c.nem >= MAX_EMITS) { EH_SET_OVERFLOW(c, 302); return; }
  blk_store(c.em, c.nem, ptr, len);
  c.nem++;
}
EH_DEV void emit_all(Ctx& c) {
  for (int i = c.cur; i < c.nb; i++) { Blk b = blk_load(c.bl, i); emit_ref(c, b.ptr, b.len); }
  c.cur = c.nb;
}
// split/1 + split_into_maxblocks/2 (erlamsa_patterns.erl:45-60) on the head of bl[cur..nb)
EH_DEV void split_head(Ctx& c) {
  if (c.cur >= c.nb) return;
  Blk h = blk_load(c.bl, c.cur);
  if (h.len <= ABSMAX_BINARY_BLOCK) return;
  // rare path: lane-uniform rebuild through bl2
  int tail = c.nb - c.cur - 1;
  for (int i = EH_LANE; i < tail; i += 64) c.bl2[i] = c.bl[c.cur + 1 + i];
  wave_sync();
  int k = c.cur; uint64_t ptr = h.ptr; uint32_t rem = h.len;
  while (rem > ABSMAX_BINARY_BLOCK) {
    uint32_t as = ABSMAXHALF_BINARY_BLOCK + rng_rand(c.rng, ABSMAXHALF_BINARY_BLOCK) - 1;
    if (k + 1 + tail >= MAX_BLOCKS) { EH_SET_OVERFLOW(c, 303); return; }
    blk_store(c.bl, k++, ptr, as); ptr += as; rem -= as;
  }
  blk_store(c.bl, k++, ptr, rem);
  if (k + tail > MAX_BLOCKS) { EH_SET_OVERFLOW(c, 304); return; }
  wave_sync();
  for (int i = EH_LANE; i < tail; i += 64) c.bl[k + i] = c.bl2[i];
  c.nb = k + tail;
  wave_sync();
}

__device__ __noinline__ void gen_force(Ctx&);   // the file / jump generators' fun, called by the pattern's first uncons (below)
enum Act { A_RUN_PAT, A_MUTATE_ONCE, A_LOOP, A_CONT, A_TERMINAL, A_DONE };
enum ContKind { C_EMIT, C_ND, C_BU, C_PAT };

// get_possible_csum_locations/1 + rand_elem (erlamsa_field_predict.erl:131-161).
// Returns 1 with (*crc,*plen,*blen), 0 for no candidate, -1 on failure.
__device__ __noinline__ int pick_csum(Ctx&, cbptr H, uint32_t L, uint32_t* crc, uint32_t* plen, uint32_t* blen) {
  EH_CTX;
  const int l = EH_LANE;
  if (L == 0) return 0;
  uint32_t maxp = (uint32_t)(2.0 * (double)L / 3.0);
  if (maxp > 30 * PREAMBLE_MAX_BYTES) maxp = 30 * PREAMBLE_MAX_BYTES;
  uint32_t np = maxp + 1;                                          // preambles 0..maxp (<= 961)
  // LDS (g_fuse_lds is free outside the fuse / sgm mutators): [0, 1024) the CRC tables wave_crc32 stages, [1024, 1024 + np) the
  // prefix CRCs, [2048, 2112) the hits as ballot masks - 16 of xor8, then 16 of crc32
  static_assert(30 * PREAMBLE_MAX_BYTES + 1 <= 1024 && 2112 <= EH_FUSE_LDS_WORDS, "pick_csum's tables fit the fuse band");
  uint32_t* T = g_fuse_lds; uint32_t* pre = g_fuse_lds + 1024; uint32_t* msk = g_fuse_lds + 2048;
  const uint32_t nbase = (np + 63) / 64;
  // xor8: xor(bytes[A .. L-1)) == byte[L-1]  <=>  prefix_xor(A) == total_xor ^ last
  uint32_t last = uni(H[L - 1]);
  uint32_t tot = wave_xor8(H, L - 1);
  uint32_t target = tot ^ last;
  wave_sync();
  uint32_t carry = 0, nx = 0;
  for (uint32_t bi = 0; bi < nbase; bi++) {
    uint32_t A = bi * 64 + (uint32_t)l;
    uint32_t v = (A < np && A < L - 1 + 1 && A > 0) ? H[A - 1] : 0;   // prefix_xor(A) = xor of bytes [0,A)
    if (A == 0 || A > L - 1) v = 0;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { uint32_t t = (uint32_t)__shfl_up((int)inc, d); if (l >= d) inc ^= t; }
    uint32_t px = inc ^ carry;
    bool hit = A < np && A <= L - 1 && px == target;               // has_xor8_checksum: needs Len - A - 1 >= 0
    const unsigned long long m = __ballot(hit);
    if (l == 0) { msk[2 * bi] = (uint32_t)m; msk[2 * bi + 1] = (uint32_t)(m >> 32); }
    nx += (uint32_t)__popcll(m);
    carry = uni((uint32_t)__shfl((int)px, 63));
  }
  // crc32: crc(bytes[A .. L-4)) == BE32(last 4), for A with L - A >= 4
  uint32_t nc = 0;
  if (L >= 4) {
    uint32_t stored = (uni(H[L - 4]) << 24) | (uni(H[L - 3]) << 16) | (uni(H[L - 2]) << 8) | uni(H[L - 1]);
    uint32_t E = L - 4;
    uint32_t whole = wave_crc32(H, E);                             // crc(0..E); the tables stay in T
    // prefix CRCs crc(0..A) for A <= maxp < 1024: lane k owns bytes [16k, 16k + 16).  The register state in front of its bytes
    // follows from the lanes before it (state' = state advanced over 16 zero bytes ^ the zero-start remainder of the 16 bytes:
    // the CRC register is linear in its start value), then every lane walks its own bytes.
    {
      const uint32_t o = 16u * (uint32_t)l;
      uint32_t by[16];
#pragma unroll
      for (int j = 0; j < 16; j++) by[j] = (o + (uint32_t)j < L && o < np) ? (uint32_t)H[o + (uint32_t)j] : 0u;
      uint32_t z = 0;                                              // zero-start remainder of my 16 bytes
#pragma unroll
      for (int j = 0; j < 16; j += 4) z = crc32_word(T, z, by[j] | (by[j + 1] << 8) | (by[j + 2] << 16) | (by[j + 3] << 24));
      uint32_t run = 0xFFFFFFFFu, mine = 0xFFFFFFFFu;
      const uint32_t nseg = (np + 15u) / 16u;
      for (uint32_t k = 0; k < nseg; k++) {
        if ((uint32_t)l == k) mine = run;
        const uint32_t zk = (uint32_t)__builtin_amdgcn_readlane((int)z, (int)k);
        run = crc32_word(T, crc32_word(T, crc32_word(T, crc32_word(T, run, 0u), 0u), 0u), 0u) ^ zk;
      }
      if (o < np) {
#pragma unroll
        for (int j = 0; j < 16; j++) {
          if (o + (uint32_t)j < np) pre[o + (uint32_t)j] = mine ^ 0xFFFFFFFFu;      // crc32(bytes[0..A))
          mine = T[(mine ^ by[j]) & 0xFFu] ^ (mine >> 8);
        }
      }
    }
    wave_sync();
    // ... then every lane tests its own preambles, from the last down: crc(A..E) = crc(0..E) ^ crc(0..A) * x^(8(E-A))
    // (crc32_combine solved for the suffix); 64 preambles further down the multiplier is x^512 times the one before
    const uint32_t x512 = gf2_xpow8n(64);
    uint32_t mul = 0; bool have = false;
    for (int bi = (int)nbase - 1; bi >= 0; bi--) {
      uint32_t A = (uint32_t)bi * 64 + (uint32_t)l;
      bool hit = false;
      if (A < np && A <= E) {
        if (!have) { mul = gf2_xpow8n(E - A); have = true; } else mul = gf2_multmodp(x512, mul);
        uint32_t suf = A == 0 ? whole : (whole ^ gf2_multmodp(mul, pre[A]));
        hit = suf == stored;
      }
      const unsigned long long m = __ballot(hit);
      if (l == 0) { msk[32 + 2 * bi] = (uint32_t)m; msk[32 + 2 * bi + 1] = (uint32_t)(m >> 32); }
      nc += (uint32_t)__popcll(m);
    }
  } else { if (l < 32) msk[32 + l] = 0; }
  wave_sync();
  uint32_t total = nx + nc;
  if (total == 0) return 0;
  uint32_t idx = rng_rand(c.rng, total);
  uint32_t want = idx, off = 0, iscrc = 0;
  if (idx >= nx) { want = idx - nx; off = 32; iscrc = 1; }
  uint32_t Asel = 0;
  for (uint32_t bi = 0; bi < nbase; bi++) {
    unsigned long long m = (unsigned long long)uni(msk[off + 2 * bi]) | ((unsigned long long)uni(msk[off + 2 * bi + 1]) << 32);
    const uint32_t cnt = (uint32_t)__popcll(m);
    if (want < cnt) { for (uint32_t t = 0; t < want; t++) m &= m - 1; Asel = bi * 64 + (uint32_t)__builtin_ctzll(m); break; }
    want -= cnt;
  }
  wave_sync();
  *crc = iscrc; *plen = Asel; *blen = iscrc ? L - Asel - 4 : L - Asel - 1;
  return 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// The container patterns (cp: gzip / zlib, ar: zip).  Both evaluate the rest of the pattern chain on a decoded payload
// (prepare4sizer(mutate_once_loop(Mutator, [], NextPat, Ip, Data, []))) and then keep using the Mutator they were GIVEN, not
// the one that evaluation returns: the scheduler's list (LaneTab), the lis / lrs / fo states and, when the result is thrown
// away, the meta trace are put back.  What is parked lives in the work area until the frame is popped.
// ---------------------------------------------------------------------------------------------------------------------
struct MutatorSave { uint32_t lt_pri[64], lt_meta[64]; uint32_t aux_save[sizeof(NestState) / 4]; int32_t nfs; uint32_t ntrace; };   // aux_save: SlotAux::nest
EH_DEV void mutator_save(Ctx& c, EH_G MutatorSave* m, uint32_t e_pri, uint32_t e_meta) {
  const int l = EH_LANE;
  m->lt_pri[l] = e_pri; m->lt_meta[l] = e_meta;
  cwptr ax = (cwptr)&c.aux->nest;
  for (int i = l; i < (int)(sizeof(NestState) / 4); i += 64) m->aux_save[i] = ax[i];
  if (l == 0) { m->nfs = c.nfs; m->ntrace = c.ntrace; }
  wave_sync();
}
EH_DEV uint64_t mutator_restore(Ctx& c, const EH_G MutatorSave* m, bool trace_too) {   // returns the lane's (e_pri, e_meta)
  const int l = EH_LANE;
  wave_sync();
  wptr ax = (wptr)&c.aux->nest;
  for (int i = l; i < (int)(sizeof(NestState) / 4); i += 64) ax[i] = m->aux_save[i];
  c.nfs = (int)uni((uint32_t)m->nfs);
  if (trace_too) c.ntrace = uni(m->ntrace);
  wave_sync();
  return ((uint64_t)m->lt_pri[l] << 32) | m->lt_meta[l];
}
// the pieces em[from..nem) as one binary (iolist_to_binary of prepare4sizer); a single piece is used where it is
EH_DEV bptr gather_emits(Ctx& c, int from, uint64_t* len) {
  uint64_t tot = 0; for (int k = from; k < c.nem; k++) tot += blk_load(c.em, k).len;
  *len = tot;
  if (tot > 0xFFFFFF00ull) { EH_SET_OVERFLOW(c, 316); return nullptr; }
  if (c.nem - from == 1) return (bptr)blk_load(c.em, from).ptr;
  bptr blob = ws_alloc_grow(c, tot + 16);
  if (!blob) return nullptr;
  uint64_t o = 0;
  for (int k = from; k < c.nem; k++) { Blk x = blk_load(c.em, k); wave_copy(blob + o, (cbptr)x.ptr, x.len); o += x.len; }
  wave_sync();
  return blob;
}

struct CpSide { MutatorSave m; Blk orig; int32_t fmt, nrest, ip, contpat; uint32_t tr_base0, pad; };   // + Blk rest[nrest]
// mutate_once_compressed/6 (erlamsa_patterns.erl:216-246) up to the inner evaluation: zlib:gunzip(Bin), on data_error
// zlib:inflate(Bin).  1: bl[cur] is the decoded Data alone and a P_CP frame waits for the evaluation; 0: not compressed
// ({Bin, Meta}); -1: the case stops (status set).
__device__ __noinline__ int cp_begin(Ctx&, uint32_t e_pri, uint32_t e_meta, EH_G PatFrame* frames, int nfr, uint32_t ip, int contpat) {
  EH_CTX;
  const int l = EH_LANE;
  const Blk b = blk_load(c.bl, c.cur);
  cbptr H = (cbptr)b.ptr;
  if (!codec_work(c, b.len)) return -1;                                      // the attempt to decode reads the block
  EH_G ZInf* zi = (EH_G ZInf*)ws_alloc_grow(c, sizeof(ZInf));
  if (!zi) return -1;
  int fmt = 0; bptr data = nullptr; uint64_t dlen = 0;
  for (int f = ZF_GZIP; f <= ZF_ZLIB && fmt == 0; f++) {
    uint64_t outn, off;
    if (!z_uncompress_size(zi, f, H, b.len, &outn, &off)) continue;
    if (outn > 0xFFFFFF00ull) { EH_SET_OVERFLOW(c, 314); return -1; }
    bptr d = ws_alloc_grow(c, outn + 16);
    if (!d) return -1;
    if (z_uncompress_write(zi, f, H, b.len, off, d, outn)) { fmt = f; data = d; dlen = outn; }
  }
  if (fmt == 0) return 0;
  if (!codec_work(c, dlen)) return -1;                                       // ... and the payload was written
  if (nfr >= MAX_FRAMES) { EH_SET_OVERFLOW(c, 315); return -1; }
  const int nrest = c.nb - c.cur - 1;
  EH_G CpSide* sd = (EH_G CpSide*)ws_alloc_grow(c, sizeof(CpSide) + (uint64_t)nrest * sizeof(Blk));
  if (!sd) return -1;
  mutator_save(c, &sd->m, e_pri, e_meta);
  // {NewBin, [{compressed, gzip}, NewMeta, {decompressed, gzip} | Meta]} :223 (zlib :241): printed as decompressed, what the payload's
  // evaluation adds (a Meta list of its own, from []), compressed
  tr_aa(c, AT_decompressed, fmt == ZF_GZIP ? AT_gzip : AT_zlib);
  const uint32_t tr_base0 = c.tr_base; c.tr_base = c.ntrace;
  EH_G Blk* rest = (EH_G Blk*)(sd + 1);
  for (int i = l; i < nrest; i += 64) rest[i] = c.bl[c.cur + 1 + i];
  if (l == 0) {
    sd->tr_base0 = tr_base0;
    sd->orig = b; sd->fmt = fmt; sd->nrest = nrest; sd->ip = (int32_t)ip; sd->contpat = contpat;
    EH_G PatFrame& f = frames[nfr];
    f.kind = P_CP; f.em_field = c.nem; f.field = (bptr)sd; f.size_bits = 0; f.big = 0; f.tail_ptr = 0; f.tail_len = 0; f.crc = 0;
  }
  wave_sync();
  blk_store(c.bl, c.cur, (uint64_t)data, (uint32_t)dlen);                   // mutate_once_loop(Mutator, [], NextPat, Ip, Data, [])
  c.nb = c.cur + 1;
  wave_sync();
  return 1;
}
// ... and after it: NewBin = zlib:gzip(NewData) | deflate(default), split({NewBin, Rest}), NewBin =:= Bin ? (:222-224,236-244,
// 252-260).  c.pat_ret 1: [NewBin | Rest] is the result (bl[cur..nb), to be written as it is); 0: unchanged - the list is
// [Bin | Rest] again, the Mutator and the trace are the ones from before, c.pat_ip / c.pat_cont say how mutate_once_loop goes
// on; -1: the case stops.  Returns the lane's scheduler entry (e_pri << 32 | e_meta) to go on with.
__device__ __noinline__ uint64_t cp_end(Ctx&, uint32_t e_pri, uint32_t e_meta, int em_field, bptr side) {
  EH_CTX;
  const int l = EH_LANE;
  const uint64_t keep = ((uint64_t)e_pri << 32) | e_meta;
  EH_G CpSide* sd = (EH_G CpSide*)side;
  const int fmt = (int)uni((uint32_t)sd->fmt), nrest = (int)uni((uint32_t)sd->nrest);
  Blk orig; orig.ptr = uni64(sd->orig.ptr); orig.len = uni(sd->orig.len); orig.aux = 0;
  c.pat_ret = -1; c.pat_ip = uni((uint32_t)sd->ip); c.pat_cont = (int)uni((uint32_t)sd->contpat);
  c.tr_base = uni(sd->tr_base0);
  tr_aa(c, AT_compressed, fmt == ZF_GZIP ? AT_gzip : AT_zlib);
  uint64_t tot;
  cbptr nd = gather_emits(c, em_field, &tot);
  if (tot > 0 && !nd) return keep;
  c.nem = em_field;
  if (!codec_work(c, tot)) return keep;                                      // zlib:gzip(NewData) | deflate
  EH_G ZDef* zd = (EH_G ZDef*)ws_alloc_grow(c, sizeof(ZDef));
  if (!zd) return keep;
  const uint64_t cap = z_deflate_bound(tot) + z_wrap_bytes(fmt);
  bptr dst = ws_alloc_grow(c, cap);
  if (!dst) return keep;
  const uint64_t nlen = z_compress(zd, fmt, nd, tot, dst, cap);
  if (nlen == 0 || nlen > 0xFFFFFF00ull) { EH_SET_OVERFLOW(c, 317); return keep; }
  const bool changed = nlen != orig.len || !wave_equal(dst, (cbptr)orig.ptr, (uint32_t)nlen);
  if (c.cur + 1 + nrest > MAX_BLOCKS) { EH_SET_OVERFLOW(c, 318); return keep; }
  const EH_G Blk* rest = (const EH_G Blk*)(sd + 1);
  wave_sync();
  for (int i = l; i < nrest; i += 64) c.bl[c.cur + 1 + i] = rest[i];
  if (changed) blk_store(c.bl, c.cur, (uint64_t)dst, (uint32_t)nlen); else blk_store(c.bl, c.cur, orig.ptr, orig.len);
  c.nb = c.cur + 1 + nrest;
  wave_sync();
  c.pat_ret = changed ? 1 : 0;
  if (changed) return keep;
  return mutator_restore(c, &sd->m, true);
}

struct ArSide { MutatorSave m; Blk archive; int32_t n, idx, ip, contpat; EH_G ZipEntry* es; uint32_t tr_base0, pad; };
// mutate_once_archiver/4 (erlamsa_patterns.erl:203-214): UnZip = zip:foldl(fun(N, I, B, Acc) -> [{N, B(), I()} | Acc] end, [], ..) over
// bl[cur] (the whole list as one binary).  c.pat_ret 1: an archive - the side block (returned) holds its entries and the Mutator;
// 0: {error, _}; -1: the case stops.
__device__ __noinline__ bptr ar_begin(Ctx&, uint32_t e_pri, uint32_t e_meta, uint32_t ip, int contpat) {
  EH_CTX;
  const Blk b = blk_load(c.bl, c.cur);
  c.pat_ret = -1;
  if (!codec_work(c, b.len)) return nullptr;                                 // zip:foldl reads the archive
  EH_G ZipRd* rd = (EH_G ZipRd*)ws_alloc_grow(c, sizeof(ZipRd));
  if (!rd) return nullptr;
  int rc = zip_open(rd, (cbptr)b.ptr, b.len);
  if (rc == ZR_UNSUP) { c.status = CASE_UNSUPPORTED; return nullptr; }
  if (rc != ZR_OK) { c.pat_ret = 0; return nullptr; }
  const uint32_t n = uni(rd->entries);
  EH_G ArSide* sd = (EH_G ArSide*)ws_alloc_grow(c, sizeof(ArSide));
  if (!sd) return nullptr;
  EH_G ZipEntry* es = (EH_G ZipEntry*)ws_alloc_grow(c, (uint64_t)(n ? n : 1) * sizeof(ZipEntry));
  if (!es) return nullptr;
  for (uint32_t i = 0; i < n; i++) {
    rc = zip_next<true>(c, rd, &es[i]);
    if (rc == ZR_STOP) return nullptr;
    if (rc == ZR_UNSUP) { c.status = CASE_UNSUPPORTED; return nullptr; }
    if (rc == ZR_CRASH) { c.status = CASE_CRASHED; return nullptr; }
    if (rc != ZR_OK) { c.pat_ret = 0; return nullptr; }
    if (!codec_work(c, uni(es[i].data_len))) return nullptr;                 // ... and inflates every file
  }
  mutator_save(c, &sd->m, e_pri, e_meta);
  if (EH_LANE == 0) { sd->archive = b; sd->n = (int32_t)n; sd->idx = (int32_t)n - 1; sd->ip = (int32_t)ip; sd->contpat = contpat; sd->es = es; }
  wave_sync();
  c.pat_ret = 1;
  return (bptr)sd;
}
// The lists:mapfoldl of mutate_once_archiver/7 (:175-186) from entry sd->idx downwards (FileSpec is in reverse central-directory
// order): R = rand(1000) per file, R > 750 runs the rest of the pattern chain on the file's bytes.  c.pat_ret 2: bl[cur] is such a
// file and a P_AR frame waits for the evaluation; 1: all files done and zip:create gave bl[cur] = NewBin; 0: zip:create failed -
// bl[cur] is the archive again, Mutator and trace are put back (the {error, _} clause, :165-174); -1: the case stops.
// Returns the lane's scheduler entry to go on with.
__device__ __noinline__ uint64_t ar_step(Ctx&, uint32_t e_pri, uint32_t e_meta, bptr side, EH_G PatFrame* frames, int nfr) {
  EH_CTX;
  const uint64_t keep = ((uint64_t)e_pri << 32) | e_meta;
  EH_G ArSide* sd = (EH_G ArSide*)side;
  EH_G ZipEntry* es = (EH_G ZipEntry*)uni64((uint64_t)sd->es);
  const int n = (int)uni((uint32_t)sd->n);
  c.pat_ret = -1; c.pat_ip = uni((uint32_t)sd->ip); c.pat_cont = (int)uni((uint32_t)sd->contpat);
  int idx = (int)uni((uint32_t)sd->idx);
  while (idx >= 0) {
    uint32_t r = rng_rand(c.rng, 1000);
    if (r > 750) {                                                                      // 25 % of the files are mutated
      if (nfr >= MAX_FRAMES) { EH_SET_OVERFLOW(c, 319); return keep; }
      blk_store(c.bl, c.cur, uni64(es[idx].data), uni(es[idx].data_len));
      c.nb = c.cur + 1;
      if (c.trace) tr_name_emit((cbptr)uni64(es[idx].name), uni(es[idx].name_len), uni(es[idx].up));   // [NM, {archiver, N} | Acc] :183: the name, then what the file's evaluation adds (a list of its own)
      if (EH_LANE == 0) sd->tr_base0 = c.tr_base;
      c.tr_base = c.ntrace;
      if (EH_LANE == 0) {
        sd->idx = idx;
        EH_G PatFrame& f = frames[nfr];
        f.kind = P_AR; f.em_field = c.nem; f.field = side; f.size_bits = 0; f.big = 0; f.tail_ptr = 0; f.tail_len = 0; f.crc = 0;
      }
      wave_sync();
      c.pat_ret = 2;
      return keep;
    }
    idx--;
  }
  if (c.work_budget) {                                                                  // zip:create deflates every file again
    uint64_t sum = 0;
    for (int i = EH_LANE; i < n; i += 64) sum += es[i].data_len;
    if (!codec_work(c, wave_sum64(sum))) return keep;
  }
  bptr out; uint64_t len;
  int rc = zip_create<true>(c, es, (uint32_t)n, &out, &len);                            // zip:create(Name, lists:reverse(NewFileSpec), [memory])
  if (rc == ZR_STOP) return keep;
  if (rc == ZR_UNSUP) { c.status = CASE_UNSUPPORTED; return keep; }
  if (rc == ZR_OK) {
    blk_store(c.bl, c.cur, (uint64_t)out, (uint32_t)len); c.nb = c.cur + 1;
    tr_aa(c, AT_archiver, AT_ok);                                                        // [{archiver, ok}, flatten(NewMeta) | Meta] :196
    wave_sync();
    c.pat_ret = 1;
    return keep;
  }
  blk_store(c.bl, c.cur, uni64(sd->archive.ptr), uni(sd->archive.len)); c.nb = c.cur + 1;
  wave_sync();
  c.pat_ret = 0;
  return mutator_restore(c, &sd->m, true);
}
// a file's evaluation ended: its pieces are the file's new bytes (prepare4sizer), the next file starts from the Mutator again
__device__ __noinline__ uint64_t ar_file_done(Ctx&, int em_field, bptr side) {
  EH_CTX;
  EH_G ArSide* sd = (EH_G ArSide*)side;
  EH_G ZipEntry* es = (EH_G ZipEntry*)uni64((uint64_t)sd->es);
  const int idx = (int)uni((uint32_t)sd->idx);
  uint64_t tot;
  bptr nb = gather_emits(c, em_field, &tot);
  c.pat_ret = -1;
  c.tr_base = uni(sd->tr_base0);
  if (!nb) return 0;
  c.nem = em_field;
  if (EH_LANE == 0) { es[idx].data = (uint64_t)nb; es[idx].data_len = (uint32_t)tot; sd->idx = idx - 1; }
  wave_sync();
  c.pat_ret = 0;
  return mutator_restore(c, &sd->m, false);
}

// The two container patterns behind one call each, so that the pattern machine (inlined into the kernel) only carries two calls.
// begin: c.pat_ret 2 = a payload is in bl[cur] and a frame was pushed; 1 = bl[cur..nb) is the pattern's result; 0 = not a
// container (go on with split/1 and mutate_once_loop); -1 = the case stops.
__device__ __noinline__ uint64_t pat_container_begin(Ctx&, uint32_t e_pri, uint32_t e_meta, int pat, EH_G PatFrame* frames, int nfr, uint32_t ip, int contpat) {
  EH_CTX;
  const uint64_t keep = ((uint64_t)e_pri << 32) | e_meta;
  if (pat == P_CP) {
    int r = cp_begin(c, e_pri, e_meta, frames, nfr, ip, contpat);
    c.pat_ret = r < 0 ? -1 : (r == 1 ? 2 : 0);
    return keep;
  }
  // list_to_binary([Bin|Rest]) -> one block
  c.pat_ret = -1;
  uint64_t tot = 0; for (int i = c.cur; i < c.nb; i++) tot += blk_load(c.bl, i).len;
  if (tot > 0xFFFFFFF0ull) { EH_SET_OVERFLOW(c, 308); return keep; }
  if (c.nb - c.cur > 1) {
    bptr all = ws_alloc_grow(c, tot);
    if (!all) return keep;
    uint64_t o = 0;
    for (int i = c.cur; i < c.nb; i++) { Blk x = blk_load(c.bl, i); wave_copy(all + o, (cbptr)x.ptr, x.len); o += x.len; }
    wave_sync();
    blk_store(c.bl, c.cur, (uint64_t)all, (uint32_t)tot); c.nb = c.cur + 1;
    wave_sync();
  }
  bptr side = ar_begin(c, e_pri, e_meta, ip, contpat);
  if (c.pat_ret != 1) return keep;
  return ar_step(c, e_pri, e_meta, side, frames, nfr);
}
// end of a payload's evaluation (the frame has been popped): c.pat_ret 2 = the next payload (ar) with a new frame; 1 = bl[cur..nb)
// is the result; 0 = go on with mutate_once_loop on bl[cur..nb) (split/1 done), c.pat_ip / c.pat_cont; -1 = the case stops.
__device__ __noinline__ uint64_t pat_container_end(Ctx&, uint32_t e_pri, uint32_t e_meta, int kind, int em_field, bptr side, EH_G PatFrame* frames, int nfr) {
  EH_CTX;
  uint64_t e;
  if (kind == P_CP) {
    e = cp_end(c, e_pri, e_meta, em_field, side);
    if (c.pat_ret < 0) return e;
    split_head(c);                                                                    // {This, LlN} = split({NewBin, Rest}) :254 (when changed, the pieces are NewBin again)
    return e;
  }
  e = ar_file_done(c, em_field, side);
  if (c.pat_ret < 0) return ((uint64_t)e_pri << 32) | e_meta;
  e = ar_step(c, (uint32_t)(e >> 32), (uint32_t)e, side, frames, nfr);
  if (c.pat_ret == 0) split_head(c);                                                  // the {error, _} clause :165-174
  return e;
}

EH_DEV void run_patterns(Ctx& c, LaneTab& lt, int pat) {
  int act = A_RUN_PAT, cont = C_EMIT, contpat = 0; uint32_t ip = 0;
  int guard = 0;
  EH_G PatFrame* frames = c.aux->frames; int nfr = 0;     // wrapper stack lives in slot memory
  while (act != A_DONE && c.status == CASE_OK) {
    if (++guard > 1000000) { EH_SET_OVERFLOW(c, 305); break; }
    switch (act) {
      case A_RUN_PAT:
        {                                                                             // [{pattern, once_dec | many_dec | burst} | Meta] :309,:326,:349; make_complex_pat's {pattern, Type} :356; nu: {pattern, no_muta} :390; co adds none
          const int pa = pat == P_OD ? AT_once_dec : pat == P_ND ? AT_many_dec : pat == P_BU ? AT_burst : pat == P_SK ? AT_skipper : pat == P_SZ ? AT_sizer : pat == P_CS ? AT_csum :
                         pat == P_AR ? AT_archiver : pat == P_CP ? AT_compressed : pat == P_NU ? AT_no_muta : -1;
          if (pa >= 0) tr_aa(c, AT_pattern, pa);
        }
        switch (pat) {
          case P_OD: cont = C_EMIT; act = A_MUTATE_ONCE; break;                       // :306-309
          case P_ND: cont = C_ND; act = A_MUTATE_ONCE; break;                         // :323-326
          case P_BU: cont = C_BU; act = A_MUTATE_ONCE; break;                         // :346-349
          case P_CO: pat = rng_erand(c.rng, 2) == 1 ? P_NU : P_OD; break;             // :378-384
          case P_NU: if (c.gen_pending) gen_force(c); split_head(c); emit_all(c); act = A_TERMINAL; break;   // :386-390
          default: {
            // make_complex_pat :351-357: the continuation pattern is drawn first, then Ip
            contpat = (int)rng_rand(c.rng, P_COUNT);                                  // rand_elem(patterns())
            cont = C_PAT;
            ip = rng_rand(c.rng, INITIAL_IP);
            if (c.gen_pending) { gen_force(c); if (c.status != CASE_OK) break; }      // uncons(Ll, false) calls a fun Ll
            if (c.cur >= c.nb) { c.status = CASE_CRASHED; break; }                    // uncons(Ll, false) -> false -> badarg
            Blk b = blk_load(c.bl, c.cur);
            cbptr H = (cbptr)b.ptr;
            if (pat == P_SK) {                                                        // mutate_once_skipper :146-161
              uint32_t len = rng_rand(c.rng, b.len / 2);
              if (c.trace) tr_kv_emit(TRK_SKIPPED, 0, 0, 0, 1, len, 0, 0);             // [{skipped, Len/8} | Meta] :154
              emit_ref(c, b.ptr, len);
              blk_store(c.bl, c.cur, b.ptr + len, b.len - len);
              wave_sync();
            } else if (pat == P_SZ) {                                                 // mutate_once_sizer :81-111
              SizerElem e;
              int r;
              {                                                                       // (out of work memory: borrow a larger area, pick again)
                const Rng rng0 = c.rng; const uint64_t mark = c.ws_used; int last_tier = 0;
                EH_PT0;
                for (;;) {
                  r = pick_simple_len(c, H, b.len, &e);
                  if (c.status != CASE_OVERFLOW || c.ovf_need == 0 || !ws_regrow(c, mark, &last_tier)) break;
                  c.rng = rng0;
                }
                EH_PT(c, PROF_PAT_PICK_LEN);
              }
              if (r < 0) break;
              if (r == 0) tr_aa(c, AT_sizer, AT_failed);                              // [{sizer, failed} | Meta] :85
              if (r == 1) {
                if (c.trace) tr_kv_emit(TRK_SIZER, 2, e.size_bits / 8, e.big ? 1u : 0u, 3, e.len, e.a, e.b);   // [{sizer, Elem} | Meta] :97
                uint32_t nbytes = e.size_bits / 8;
                if ((uint64_t)e.a + nbytes + e.len > b.len) { c.status = CASE_CRASHED; break; }
                if (nfr >= MAX_FRAMES) { EH_SET_OVERFLOW(c, 306); break; }
                bptr fld = ws_alloc_grow(c, 16);
                if (!fld) break;
                emit_ref(c, b.ptr, e.a);                                              // H
                if (EH_LANE == 0) {
                  EH_G PatFrame& f = frames[nfr];
                  f.kind = P_SZ; f.em_field = c.nem; f.field = fld; f.size_bits = e.size_bits; f.big = e.big;
                  f.tail_ptr = b.ptr + e.a + nbytes + e.len; f.tail_len = b.len - (e.a + nbytes + e.len); f.crc = 0;
                }
                nfr++;
                emit_ref(c, (uint64_t)fld, nbytes);                                   // length field, filled when the inner evaluation ends
                blk_store(c.bl, c.cur, b.ptr + e.a + nbytes, e.len);                  // Blob
                wave_sync();
              }
            } else if (pat == P_CS) {                                                 // mutate_once_csum :115-144
              uint32_t iscrc, plen, blen;
              EH_PT0;
              int r = pick_csum(c, H, b.len, &iscrc, &plen, &blen);
              EH_PT(c, PROF_PAT_PICK_CSUM);
              if (r < 0) break;
              if (r == 0) tr_aa(c, AT_csum, AT_failed);                               // :119
              if (r == 1) {
                if (c.trace) tr_kv_emit(TRK_CSUM, 1, iscrc, 0, 2, plen, blen, 0);      // [{csum, Elem} | Meta] :131
                if (nfr >= MAX_FRAMES) { EH_SET_OVERFLOW(c, 307); break; }
                emit_ref(c, b.ptr, plen);                                             // P
                if (EH_LANE == 0) {
                  EH_G PatFrame& f = frames[nfr];
                  f.kind = P_CS; f.em_field = c.nem; f.crc = iscrc; f.field = nullptr; f.size_bits = 0; f.big = 0; f.tail_ptr = 0; f.tail_len = 0;
                }
                nfr++;
                blk_store(c.bl, c.cur, b.ptr + plen, blen);
                wave_sync();
              }
            } else if (pat == P_AR || pat == P_CP) {                                  // mutate_once_archiver :165-214, mutate_once_compressed :216-260
              EH_PT0;
              uint64_t e = pat_container_begin(c, lt.e_pri, lt.e_meta, pat, frames, nfr, ip, contpat);
              EH_PT(c, pat == P_CP ? PROF_PAT_CP_BEGIN : PROF_PAT_AR_BEGIN);
              lt.e_pri = (uint32_t)(e >> 32); lt.e_meta = (uint32_t)e;
              if (c.pat_ret < 0) break;
              if (c.pat_ret == 2) { nfr++; act = A_LOOP; break; }                     // the rest of the chain on a payload: mutate_once_loop(Mutator, [], NextPat, Ip, Data, [])
              if (c.pat_ret == 1) { emit_all(c); act = A_TERMINAL; break; }           // [NewBin | {..}]
              tr_aa(c, pat == P_CP ? AT_compressed : AT_archiver, AT_failed);         // [{compressed, failed} | Meta] :259 / [{archiver, failed} | Meta] :169
            }
            split_head(c);
            act = A_LOOP;
            break;
          }
        }
        break;
      case A_MUTATE_ONCE:                                                             // mutate_once/4 :265-278
        if (!c.gen_pending && c.nb - c.cur == 1 && blk_load(c.bl, c.cur).len == 0) { tr_aa(c, AT_mutate_once, AT_empty_stopped); c.cur = c.nb; act = A_TERMINAL; break; }   // {Mutator, [{mutate_once, empty_stopped} | Meta]} :268-269 (a fun does not match [<<>>])
        ip = rng_rand(c.rng, INITIAL_IP);
        if (c.gen_pending) { gen_force(c); if (c.status != CASE_OK) break; }          // uncons(Ll, false) calls a fun Ll
        if (c.cur >= c.nb) { act = A_CONT; break; }                                   // Cont([], ...)
        split_head(c);
        act = A_LOOP;
        break;
      case A_LOOP: {                                                                  // mutate_once_loop/6 :281-296
        uint32_t n = rng_rand(c.rng, ip);
        if (n == 0 || c.nb - c.cur == 1) { mux_fuzzers(c, lt); act = A_CONT; }
        else { Blk b = blk_load(c.bl, c.cur); emit_ref(c, b.ptr, b.len); c.cur++; }
        break;
      }
      case A_CONT:
        switch (cont) {
          case C_EMIT: emit_all(c); act = A_TERMINAL; break;
          case C_ND:                                                                  // pat_many_dec_cont :313-321
            if (rng_occurs(c.rng, 4, 5)) { tr_aa(c, AT_pattern, AT_many_dec); act = A_MUTATE_ONCE; } else { emit_all(c); act = A_TERMINAL; }
            break;
          case C_BU: {                                                                // pat_burst_cont :331-344
            int n = 1;
            while (c.status == CASE_OK) {
              bool p = rng_occurs(c.rng, 4, 5);
              if (p || n < 2) { mux_fuzzers(c, lt); n++; } else { emit_all(c); act = A_TERMINAL; break; }
              if (++guard > 1000000) { EH_SET_OVERFLOW(c, 309); break; }
            }
            break;
          }
          case C_PAT: pat = contpat; act = A_RUN_PAT; break;
        }
        break;
      case A_TERMINAL: {
        // the innermost evaluation finished: unwind the sizer/csum wrappers inside out
        if (nfr == 0) { act = A_DONE; break; }
        wave_sync();
        PatFrame f = frames[--nfr];
        f.kind = (int)uni((uint32_t)f.kind); f.em_field = (int)uni((uint32_t)f.em_field); f.field = (bptr)uni64((uint64_t)f.field);
        f.size_bits = uni(f.size_bits); f.big = uni(f.big); f.tail_ptr = uni64(f.tail_ptr); f.tail_len = uni(f.tail_len); f.crc = uni(f.crc);
        if (f.kind == P_AR || f.kind == P_CP) {
          EH_PT0;
          uint64_t e = pat_container_end(c, lt.e_pri, lt.e_meta, f.kind, f.em_field, f.field, frames, nfr);
          EH_PT(c, f.kind == P_CP ? PROF_PAT_CP_END : PROF_PAT_AR_END);
          lt.e_pri = (uint32_t)(e >> 32); lt.e_meta = (uint32_t)e;
          if (c.pat_ret < 0) break;
          ip = c.pat_ip; cont = C_PAT; contpat = c.pat_cont;
          if (c.pat_ret == 2) { nfr++; act = A_LOOP; }                                // ar: the next file's evaluation
          else if (c.pat_ret == 1) emit_all(c);                                       // [NewBin | Rest] ++ [..]: no continuation
          else { tr_aa(c, f.kind == P_CP ? AT_compressed : AT_archiver, AT_failed); act = A_LOOP; }   // unchanged / zip:create failed: mutate_once_loop(Mutator, [{compressed | archiver, failed} | Meta], NextPat, Ip, This, LlN) - the Meta from before the pattern (mutator_restore)
        } else if (f.kind == P_SZ) {
          // NewLen = size(NewBlob) = everything written after the length field  (:105-110)
          uint64_t tot = 0; for (int k = f.em_field + 1; k < c.nem; k++) tot += blk_load(c.em, k).len;
          // (the field piece itself is at em_field unless Size/8 was 0, which cannot happen)
          if (EH_LANE == 0) put_field(f.field, tot, f.size_bits, f.big != 0);
          wave_sync();
          emit_ref(c, f.tail_ptr, f.tail_len);                                        // TailBin
        } else {
          // NewC = recalc_csum(Type, NewBlob): gather the inner pieces, checksum, append  (:139-143)
          uint64_t tot = 0; for (int k = f.em_field; k < c.nem; k++) tot += blk_load(c.em, k).len;
          if (tot > 0xFFFFFFF0ull) { EH_SET_OVERFLOW(c, 310); break; }
          EH_PT0;
          bptr blob = ws_alloc_grow(c, tot + 16);
          if (!blob) break;
          uint64_t o = 0;
          for (int k = f.em_field; k < c.nem; k++) { Blk x = blk_load(c.em, k); wave_copy(blob + o, (cbptr)x.ptr, x.len); o += x.len; }
          wave_sync();
          EH_PT(c, PROF_PAT_CS_BLOB);
          uint32_t cs = f.crc ? wave_crc32(blob, (uint32_t)tot) : wave_xor8(blob, (uint32_t)tot);
          EH_PT(c, PROF_PAT_CS_SUM);
          uint32_t cb = f.crc ? 4u : 1u;
          if (EH_LANE == 0) put_field(blob + tot, cs, cb * 8, true);
          wave_sync();
          c.nem = f.em_field;
          emit_ref(c, (uint64_t)blob, (uint32_t)tot + cb);
        }
        break;
      }
    }
  }
}
