// eh_gen.h - device: the generators (erlamsa_gen.erl).  A part of eh_engine.hip, included there once, inside namespace eh,
// behind eh_patterns.h and in front of co_exec.
#pragma once
// =============================================================================================
// device: generators
// =============================================================================================
// finish/1 (erlamsa_gen.erl:43-51): with probability 1/(Len+1) a block of random bytes behind the stream, at bl[c.nb]
EH_DEV void gen_finish(Ctx& c, uint32_t len) {
  uint32_t n = rng_rand(c.rng, len + 1);
  if (n == len) {
    uint32_t bits = rng_range(c.rng, 1, 16);
    uint32_t nlen = rng_rand(c.rng, 1u << bits);
    if (nlen > 0) {                                                    // check_empty
      bptr dst = ws_alloc_grow(c, nlen);
      if (!dst) return;
      random_block_rev(c, dst, nlen);
      if (c.nb >= MAX_BLOCKS) { EH_SET_OVERFLOW(c, 312); return; }
      blk_store(c.bl, c.nb, (uint64_t)dst, nlen);
      c.nb++;
    }
  }
}
EH_DEV uint32_t rand_block_size(Ctx& c) {                              // :55-56
  uint32_t r = rng_rand(c.rng, c.max_block_scaled);
  return r > c.min_block_scaled ? r : c.min_block_scaled;
}
EH_DEV void gen_direct(Ctx& c, cbptr in, uint32_t L) {       // erlamsa_gen.erl:152-164 (split_binary guard never holds)
  (void)rand_block_size(c);
  blk_store(c.bl, 0, (uint64_t)in, L);
  c.nb = 1;
  gen_finish(c, L);
  wave_sync();
}
// port_stream/2 forced (erlamsa_gen.erl:59-90) over corpus entry e: the blocks point into the arena (nothing is copied), the
// next block size is drawn after every full block, a short read is followed by eof and finish(Len).  Fills bl[0..nb).
EH_DEV void gen_stream(Ctx& c, uint32_t e) {
  const EH_G KParams& p = *c.p;
  uint64_t o0 = uni64(p.coff[e]), o1 = uni64(p.coff[e + 1]);
  cbptr in = p.corpus + o0;
  uint32_t L = (uint32_t)(o1 - o0), pos = 0;
  c.nb = 0;
  uint32_t wanted = rand_block_size(c);
  while (pos < L) {
    if (c.nb >= MAX_BLOCKS - 1) { EH_SET_OVERFLOW(c, 313); return; }
    uint32_t avail = L - pos;
    if (avail >= wanted) { blk_store(c.bl, c.nb++, (uint64_t)(in + pos), wanted); pos += wanted; wanted = rand_block_size(c); }
    else { blk_store(c.bl, c.nb++, (uint64_t)(in + pos), avail); pos = L; }
  }
  gen_finish(c, L);
  wave_sync();
}
// The file and jump generators hand the pattern a FUN (file_streamer :106-121, jump_streamer :136-150): only the paths are
// drawn when DataGen() runs; the streams are read, and their block sizes drawn, when the pattern's first uncons/2 calls the
// fun (erlamsa_utils.erl:93) - after the pattern's own first draws.  gen_force is that call.
__device__ __noinline__ void gen_force(Ctx&) {
  EH_CTX;
  const int kind = c.gen_pending;
  c.gen_pending = 0;
  if (kind == G_FILE) { gen_stream(c, c.gen_e1); return; }
  // jump_somewhere/2 :124-133
  uint64_t dptr[2]; uint32_t dlen[2];
  for (int k = 0; k < 2; k++) {
    gen_stream(c, k == 0 ? c.gen_e1 : c.gen_e2);
    if (c.status != CASE_OK) return;
    if (c.nb == 0) { c.status = CASE_CRASHED; return; }                // rand_elem([]) = [] ; size([]) -> badarg
    uint32_t i = rng_erand(c.rng, (uint32_t)c.nb) - 1;                 // rand_elem/1 (erlamsa_rnd.erl:128-132)
    Blk b = blk_load(c.bl, (int)i);
    dptr[k] = b.ptr; dlen[k] = b.len;
    wave_sync();
  }
  uint32_t s1 = rng_rand(c.rng, dlen[0]), s2 = rng_rand(c.rng, dlen[1]);
  uint32_t l1 = rng_erand(c.rng, dlen[0] - s1), l2 = rng_erand(c.rng, dlen[1] - s2);
  bptr dst = ws_alloc_grow(c, (uint64_t)l1 + l2);
  if (!dst) return;
  wave_copy(dst, (cbptr)dptr[0] + s1, l1);
  wave_copy(dst + l1, (cbptr)dptr[1] + s2, l2);
  wave_sync();
  blk_store(c.bl, 0, (uint64_t)dst, l1 + l2);                          // uncons(B) when is_binary(B) -> {B, []}
  c.nb = 1;
  wave_sync();
}
EH_DEV void gen_random(Ctx& c) {                                       // random_stream/1 :167-178
  c.nb = 0;
  while (c.status == CASE_OK) {
    uint32_t n = rng_range(c.rng, 32, c.max_block_scaled);
    bptr dst = ws_alloc_grow(c, n);
    if (!dst) return;
    random_block_rev(c, dst, n);
    if (c.nb >= MAX_BLOCKS) { EH_SET_OVERFLOW(c, 311); return; }
    blk_store(c.bl, c.nb++, (uint64_t)dst, n);
    uint32_t ip = rng_range(c.rng, 1, 100);
    if (rng_rand(c.rng, ip) == 0) break;
  }
  wave_sync();
}
