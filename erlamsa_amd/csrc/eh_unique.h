// eh_unique.h — the uniqueness filter of a batch's results: per-case digests, duplicate detection, on the device
// (include/erlamsa_hip.h: eh_result_digests, eh_result_unique, eh_result_download_select, eh_selftest_unique).
//
// What it stands for on the reference side: radamsa's --hash / --checksums filter, which erlamsa restates without one.  The bytes
// are on the device, and a duplicate that is found there never crosses PCIe.
//
//   digest(i) = (uint64) crc32c(out_i) << 32 | crc32(out_i)         (both reflected, init and final xor 0xFFFFFFFF; empty -> 0)
//
// Both CRCs are linear over GF(2): crc(A ++ B) = crc(A) * x^(8 |B|) ^ crc(B), so pieces of one case are hashed by different
// wavefronts and put together afterwards.  Work is cut by BYTES: a case is UQ_PIECE-byte pieces (the last one shorter), the pieces
// of all cases are numbered by a scan over the lengths (piece_first), and wavefronts take piece numbers grid-stride.  A
// wavefront-per-case kernel would serialise exactly where the bytes are (1 % of the cases of the bench workload carry 83 % of them).
//
// Launches, all on the context's stream, none waits for another workgroup:
//   eh_uq_scan_kernel      piece_first[i] = pieces in front of case i                        (one wavefront, like eh_order_scan_kernel)
//   eh_uq_digest_kernel    term[p] = both CRCs of piece p                                    (reads the arena once)
//   eh_uq_combine_kernel   digest[i] = xor of term[p] * x^(8 * bytes of the case behind p)   (store, then reduce: no order, no atomics)
//   eh_uq_init_kernel      hash table empty, counters zero
//   eh_uq_insert_kernel    one lane per EH_CASE_OK case: claims / finds the slot of its (length, digest), atomicMin of the case index
//   eh_uq_resolve_kernel   first_of[i] = smallest case index of the slot
//   eh_uq_compare_kernel   piece by piece again: a non-representative case against its representative, atomicOr of a mismatch flag
//   eh_uq_final_kernel     a flagged case is its own first; counts the unique cases and their bytes
#pragma once
#include "eh_zlib.h"

namespace eh {

constexpr uint32_t UQ_PIECE = 65536;                 // bytes of a piece (eh_selftest_unique reports it: tests do not guess)
constexpr uint32_t UQ_SUB = UQ_PIECE / 64;           // a lane's share of a full piece
constexpr uint32_t UQ_POLY_CRC32 = 0xEDB88320u, UQ_POLY_CRC32C = 0x82F63B78u;
constexpr uint64_t UQ_EMPTY = ~0ull;
static_assert(UQ_SUB % 16 == 0, "a lane's share is whole 16-byte loads");

// a(x) * b(x) mod p(x), reflected representation (x^0 = bit 31); gf2_multmodp of eh_zlib.h for either polynomial, and safe for a == 0
constexpr uint32_t uq_mul(uint32_t poly, uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m && (a & (m | (m - 1))); m >>= 1) { if (a & m) p ^= b; b = (b & 1) ? (b >> 1) ^ poly : b >> 1; }
  return p;
}
struct alignas(16) UqTabs {
  uint32_t pow[2][64];      // x^(8 * 2^k)
  uint32_t lane[2][64];     // x^(8 * UQ_SUB * (63 - l)): what lies behind lane l's share of a full piece
  uint32_t head[2][16];     // x^(8 * (UQ_SUB - h)): a full piece whose first h bytes go to lane 0 as a scalar head (below)
};
constexpr UqTabs uq_tabs() {
  UqTabs t{};
  const uint32_t poly[2] = {UQ_POLY_CRC32, UQ_POLY_CRC32C};
  for (int c = 0; c < 2; c++) {
    uint32_t sq = 1u << 23;                                          // x^8
    for (int k = 0; k < 64; k++) { t.pow[c][k] = sq; sq = uq_mul(poly[c], sq, sq); }
    uint32_t xs = 1u << 31;                                          // x^(8 * UQ_SUB)
    for (int k = 0; k < 64; k++) if ((UQ_SUB >> k) & 1) xs = uq_mul(poly[c], xs, t.pow[c][k]);
    t.lane[c][63] = 1u << 31;
    for (int l = 62; l >= 0; l--) t.lane[c][l] = uq_mul(poly[c], t.lane[c][l + 1], xs);
    uint32_t v = 1u << 31;                                           // x^(8 * (UQ_SUB - h)), from h = UQ_SUB down
    uint32_t tmp[UQ_SUB + 1] = {};
    for (uint32_t k = 0; k <= UQ_SUB; k++) { tmp[k] = v; v = uq_mul(poly[c], v, 1u << 23); }
    for (int h = 0; h < 16; h++) t.head[c][h] = tmp[UQ_SUB - h];
  }
  return t;
}
__constant__ UqTabs c_uq_tabs = uq_tabs();
constexpr TabU32x1024 uq_slices(uint32_t poly) {
  TabU32x1024 t{};
  for (uint32_t i = 0; i < 256; i++) { uint32_t cc = i; for (int k = 0; k < 8; k++) cc = (cc & 1) ? poly ^ (cc >> 1) : cc >> 1; t.v[i] = cc; }
  for (int k = 1; k < 4; k++) for (uint32_t i = 0; i < 256; i++) { uint32_t q = t.v[(k - 1) * 256 + i]; t.v[k * 256 + i] = (q >> 8) ^ t.v[q & 0xFF]; }
  return t;
}
__constant__ TabU32x1024 c_uq_crc32c_slices = uq_slices(UQ_POLY_CRC32C);     // (CRC-32's are c_crc_slices of eh_zlib.h)

// the slicing tables of both CRCs, 8 KiB of the digest kernel's own LDS (g_fuse_lds is the mutate kernel's)
EH_LDS_ARRAY(uint32_t, g_uq_lds, 2048);

EH_DEV uint32_t uq_xpow8n(int c, uint64_t nbytes) {                  // x^(8 * nbytes) mod p, from the table of squares
  const uint32_t poly = c ? UQ_POLY_CRC32C : UQ_POLY_CRC32;
  uint32_t r = 1u << 31;
  for (int k = 0; nbytes; k++, nbytes >>= 1) if (nbytes & 1) r = uq_mul(poly, r, c_uq_tabs.pow[c][k]);
  return r;
}
EH_DEV uint32_t uq_wave_xor(uint32_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d);
  return v;
}
EH_DEV uint64_t uq_wave_add64(uint64_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1)
    v += ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, d);
  return v;
}
EH_DEV uint64_t uq_pieces_of(uint64_t len) { return (len + (UQ_PIECE - 1)) / UQ_PIECE; }

// piece_first[i] = pieces of the cases in front of case i, piece_first[n] = all pieces: one wavefront, 64 cases per step
__global__ void __launch_bounds__(64) eh_uq_scan_kernel(const uint64_t* out_len_, uint64_t* piece_first_, uint64_t n) {
  cqptr out_len = (cqptr)out_len_; qptr piece_first = (qptr)piece_first_;
  const int l = EH_LANE;
  uint64_t run = 0;
  for (uint64_t base = 0; base < n; base += 64) {
    uint64_t i = base + (uint64_t)l;
    uint64_t v = i < n ? uq_pieces_of(out_len[i]) : 0;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      uint64_t t = ((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(inc >> 32), d) << 32) | (uint32_t)__shfl_up((int)(uint32_t)inc, d);
      if (l >= d) inc += t;
    }
    if (i < n) piece_first[i] = run + inc - v;
    run += uni64(((uint64_t)(uint32_t)__shfl((int)(uint32_t)(inc >> 32), 63) << 32) | (uint32_t)__shfl((int)(uint32_t)inc, 63));
  }
  if (l == 0) piece_first[n] = run;
}
// the case piece p belongs to: piece_first[i] <= p < piece_first[i + 1] (cases without bytes have no piece and are never found)
EH_DEV uint64_t uq_case_of(cqptr piece_first, uint64_t n, uint64_t p) {
  uint64_t lo = 0, hi = n;
  while (hi - lo > 1) { uint64_t mid = lo + ((hi - lo) >> 1); if (piece_first[mid] <= p) lo = mid; else hi = mid; }
  return lo;
}

// term[p] = crc32c << 32 | crc32 of piece p alone.  Every lane owns a contiguous share; all shares but lane 0's begin at an
// address that is a multiple of 16 (lane 0 takes the h = -address mod 16 bytes in front as a scalar head), so the loads are aligned
// dwordx4 wherever the case begins in the arena, and what is left at a share's end is a scalar tail.
__global__ void __launch_bounds__(64) eh_uq_digest_kernel(const uint8_t* data_, const uint64_t* out_off_, const uint64_t* out_len_, const uint64_t* piece_first_,
                                                          uint64_t n, unsigned long long* term_, uint64_t term_cap) {
  cbptr data = (cbptr)data_; cqptr out_off = (cqptr)out_off_, out_len = (cqptr)out_len_, piece_first = (cqptr)piece_first_;
  EH_G unsigned long long* term = (EH_G unsigned long long*)term_;
  const int l = EH_LANE;
  uint32_t* T = g_uq_lds;
  for (int i = l; i < 1024; i += 64) { T[i] = c_crc_slices.v[i]; T[1024 + i] = c_uq_crc32c_slices.v[i]; }
  wave_sync();
  uint64_t np = uni64(piece_first[n]); if (np > term_cap) np = term_cap;
  for (uint64_t p = blockIdx.x; p < np; p += gridDim.x) {
    const uint64_t i = uni64(uq_case_of(piece_first, n, p));
    const uint64_t len = uni64(out_len[i]), done = (p - uni64(piece_first[i])) * UQ_PIECE;
    const uint32_t plen = len - done > UQ_PIECE ? UQ_PIECE : (uint32_t)(len - done);
    cbptr src = data + uni64(out_off[i]) + done;
    const bool full = plen == UQ_PIECE;
    const uint32_t chunk = full ? UQ_SUB : (((plen + 63) / 64) + 15) & ~15u;
    uint32_t h = (uint32_t)((16 - ((uintptr_t)src & 15)) & 15); if (h > plen) h = plen;
    uint32_t a = l ? h + (uint32_t)l * chunk : 0, b = l == 63 ? plen : h + ((uint32_t)l + 1) * chunk;
    if (a > plen) a = plen;
    if (b > plen) b = plen;
    uint32_t c1 = 0xFFFFFFFFu, c2 = 0xFFFFFFFFu;
    uint32_t k = a;
    if (l == 0) for (; k < h; k++) { const uint32_t x = src[k]; c1 = T[(c1 ^ x) & 0xFF] ^ (c1 >> 8); c2 = T[1024 + ((c2 ^ x) & 0xFF)] ^ (c2 >> 8); }
    if (k + 16 <= b) {
      uint4 w = ldg16a(src + k);
      for (; k + 32 <= b; k += 16) {
        const uint4 nx = ldg16a(src + k + 16);                       // the next load is in flight while this one is folded in
        c1 = crc32_word(T, c1, w.x); c2 = crc32_word(T + 1024, c2, w.x); c1 = crc32_word(T, c1, w.y); c2 = crc32_word(T + 1024, c2, w.y);
        c1 = crc32_word(T, c1, w.z); c2 = crc32_word(T + 1024, c2, w.z); c1 = crc32_word(T, c1, w.w); c2 = crc32_word(T + 1024, c2, w.w);
        w = nx;
      }
      c1 = crc32_word(T, c1, w.x); c2 = crc32_word(T + 1024, c2, w.x); c1 = crc32_word(T, c1, w.y); c2 = crc32_word(T + 1024, c2, w.y);
      c1 = crc32_word(T, c1, w.z); c2 = crc32_word(T + 1024, c2, w.z); c1 = crc32_word(T, c1, w.w); c2 = crc32_word(T + 1024, c2, w.w);
      k += 16;
    }
    for (; k < b; k++) { const uint32_t x = src[k]; c1 = T[(c1 ^ x) & 0xFF] ^ (c1 >> 8); c2 = T[1024 + ((c2 ^ x) & 0xFF)] ^ (c2 >> 8); }
    c1 ^= 0xFFFFFFFFu; c2 ^= 0xFFFFFFFFu;                            // the CRCs of my share (0 and 0 for an empty one)
    if (a >= b) { c1 = 0; c2 = 0; }
    // crc32_combine over the 64 shares: share l contributes crc_l * x^(8 * bytes of the piece behind it)
    uint32_t t1, t2;
    if (full) {
      // behind lane l < 63: (63 - l) * UQ_SUB - h bytes = x^(8 UQ_SUB (62 - l)) * x^(8 (UQ_SUB - h)): a table entry per lane, and one
      // factor for the whole wavefront
      const uint32_t m1 = l < 63 ? uq_mul(UQ_POLY_CRC32, c_uq_tabs.lane[0][l + 1], c1) : 0u, m2 = l < 63 ? uq_mul(UQ_POLY_CRC32C, c_uq_tabs.lane[1][l + 1], c2) : 0u;
      const uint32_t s1 = uq_wave_xor(m1), s2 = uq_wave_xor(m2);
      const uint32_t e1 = (uint32_t)__shfl((int)c1, 63), e2 = (uint32_t)__shfl((int)c2, 63);
      t1 = uq_mul(UQ_POLY_CRC32, c_uq_tabs.head[0][h], s1) ^ e1; t2 = uq_mul(UQ_POLY_CRC32C, c_uq_tabs.head[1][h], s2) ^ e2;
    } else {
      const uint32_t m1 = a < b ? uq_mul(UQ_POLY_CRC32, uq_xpow8n(0, plen - b), c1) : 0u, m2 = a < b ? uq_mul(UQ_POLY_CRC32C, uq_xpow8n(1, plen - b), c2) : 0u;
      t1 = uq_wave_xor(m1); t2 = uq_wave_xor(m2);
    }
    if (l == 0) term[p] = ((unsigned long long)t2 << 32) | t1;
  }
}

// digest[i] = xor over the pieces of case i of term[p] * x^(8 * bytes of the case behind piece p).  64 cases per step, a lane per
// case; a case of more than 4 pieces is then taken by the whole wavefront, a lane per piece.
EH_DEV uint64_t uq_shift_term(uint64_t t, uint64_t behind) {
  if (!behind) return t;
  return ((uint64_t)uq_mul(UQ_POLY_CRC32C, uq_xpow8n(1, behind), (uint32_t)(t >> 32)) << 32) | uq_mul(UQ_POLY_CRC32, uq_xpow8n(0, behind), (uint32_t)t);
}
__global__ void __launch_bounds__(64) eh_uq_combine_kernel(const uint64_t* out_len_, const uint64_t* piece_first_, uint64_t n, const unsigned long long* term_, uint64_t term_cap,
                                                           uint64_t* digest_) {
  cqptr out_len = (cqptr)out_len_, piece_first = (cqptr)piece_first_; qptr digest = (qptr)digest_;
  const EH_G unsigned long long* term = (const EH_G unsigned long long*)term_;
  const int l = EH_LANE;
  for (uint64_t base = (uint64_t)blockIdx.x * 64; base < n; base += (uint64_t)gridDim.x * 64) {
    const uint64_t i = base + (uint64_t)l;
    uint64_t p0 = 0, p1 = 0, len = 0;
    if (i < n) { p0 = piece_first[i]; p1 = piece_first[i + 1]; len = out_len[i]; if (p1 > term_cap) p1 = term_cap; if (p0 > p1) p0 = p1; }
    const bool big = p1 - p0 > 4;
    if (i < n && !big) {
      uint64_t d = 0;
      for (uint64_t p = p0; p < p1; p++) { const uint64_t end = (p - p0 + 1) * UQ_PIECE; d ^= uq_shift_term(term[p], end < len ? len - end : 0); }
      digest[i] = d;
    }
    unsigned long long todo = __ballot(big);
    while (todo) {
      const int src = __builtin_ctzll(todo); todo &= todo - 1;
      const uint64_t q0 = uni64(((uint64_t)(uint32_t)__shfl((int)(uint32_t)(p0 >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)p0, src));
      const uint64_t q1 = uni64(((uint64_t)(uint32_t)__shfl((int)(uint32_t)(p1 >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)p1, src));
      const uint64_t ql = uni64(((uint64_t)(uint32_t)__shfl((int)(uint32_t)(len >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)len, src));
      uint64_t d = 0;
      for (uint64_t p = q0 + (uint64_t)l; p < q1; p += 64) { const uint64_t end = (p - q0 + 1) * UQ_PIECE; d ^= uq_shift_term(term[p], end < ql ? ql - end : 0); }
      const uint32_t lo = uq_wave_xor((uint32_t)d), hi = uq_wave_xor((uint32_t)(d >> 32));
      if (l == 0) digest[base + (uint64_t)src] = ((uint64_t)hi << 32) | lo;
    }
  }
}

// ---- duplicates ---------------------------------------------------------------------------------------------------------------
// Open addressing, `slots` (a power of two, at least 2 n) entries: owner[s] = a case whose (length, digest) the slot stands for - the
// first that claimed it, whichever that was; the key is read through it, the arrays it sits in do not change - and rep[s] = the
// smallest index among the EH_CASE_OK cases with that key, whatever the scheduling (atomicMin).
__global__ void __launch_bounds__(64) eh_uq_init_kernel(unsigned long long* tab_, uint64_t nwords) {
  EH_G unsigned long long* tab = (EH_G unsigned long long*)tab_;
  for (uint64_t k = (uint64_t)blockIdx.x * 64 + (uint64_t)EH_LANE; k < nwords; k += (uint64_t)gridDim.x * 64) tab[k] = k < 2 ? 0ull : UQ_EMPTY;   // [0] unique cases, [1] their bytes
}
EH_DEV uint64_t uq_hash(uint64_t len, uint64_t dig) {
  uint64_t x = dig ^ (len * 0x9E3779B97F4A7C15ull);
  x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 32;
  return x;
}
__global__ void __launch_bounds__(64) eh_uq_insert_kernel(const uint64_t* out_len_, const int32_t* status_, const uint64_t* digest_, uint64_t n,
                                                          unsigned long long* owner_, unsigned long long* rep_, uint64_t slots, uint64_t* first_of_) {
  cqptr out_len = (cqptr)out_len_, digest = (cqptr)digest_; const EH_G int32_t* status = (const EH_G int32_t*)status_; qptr first_of = (qptr)first_of_;
  EH_G unsigned long long* owner = (EH_G unsigned long long*)owner_; EH_G unsigned long long* rep = (EH_G unsigned long long*)rep_;
  for (uint64_t i = (uint64_t)blockIdx.x * 64 + (uint64_t)EH_LANE; i < n; i += (uint64_t)gridDim.x * 64) {
    if (status[i] != CASE_OK) { first_of[i] = UQ_EMPTY; continue; }
    const uint64_t len = out_len[i], dig = digest[i];
    uint64_t s = uq_hash(len, dig) & (slots - 1);
    for (uint64_t tries = 0; tries < slots; tries++, s = (s + 1) & (slots - 1)) {      // (at most n of the >= 2 n slots are ever taken)
      unsigned long long o = owner[s];
      if (o == UQ_EMPTY) { o = atomicCAS(&owner[s], (unsigned long long)UQ_EMPTY, (unsigned long long)i); if (o == UQ_EMPTY) o = i; }
      if (out_len[o] == len && digest[o] == dig) { atomicMin(&rep[s], (unsigned long long)i); break; }
    }
    first_of[i] = s;
  }
}
__global__ void __launch_bounds__(64) eh_uq_resolve_kernel(const unsigned long long* rep_, uint64_t n, uint64_t* first_of_, uint32_t* flag_) {
  const EH_G unsigned long long* rep = (const EH_G unsigned long long*)rep_; qptr first_of = (qptr)first_of_; wptr flag = (wptr)flag_;
  for (uint64_t i = (uint64_t)blockIdx.x * 64 + (uint64_t)EH_LANE; i < n; i += (uint64_t)gridDim.x * 64) {
    const uint64_t s = first_of[i];
    const uint64_t r = s == UQ_EMPTY ? i : (uint64_t)rep[s];
    first_of[i] = r < i ? r : i;
    flag[i] = 0;
  }
}
// Same length and same digest are not yet the same bytes: every case that is not its key's first is compared with it, cut into
// the digest pass's pieces, so that two equal outputs of a gigabyte are not one wavefront's work.
__global__ void __launch_bounds__(64) eh_uq_compare_kernel(const uint8_t* data_, const uint64_t* out_off_, const uint64_t* out_len_, const uint64_t* piece_first_,
                                                           uint64_t n, const uint64_t* first_of_, uint32_t* flag_) {
  cbptr data = (cbptr)data_; cqptr out_off = (cqptr)out_off_, out_len = (cqptr)out_len_, piece_first = (cqptr)piece_first_, first_of = (cqptr)first_of_;
  wptr flag = (wptr)flag_;
  const uint64_t np = uni64(piece_first[n]);
  for (uint64_t p = blockIdx.x; p < np; p += gridDim.x) {
    const uint64_t i = uni64(uq_case_of(piece_first, n, p));
    const uint64_t r = uni64(first_of[i]);
    if (r >= i) continue;                                            // its key's first (or not EH_CASE_OK: first_of[i] = i)
    const uint64_t len = uni64(out_len[i]), done = (p - uni64(piece_first[i])) * UQ_PIECE;
    if (uni64(out_len[r]) != len) continue;                          // (cannot be: the key holds the length)
    const uint32_t plen = len - done > UQ_PIECE ? UQ_PIECE : (uint32_t)(len - done);
    const bool eq = wave_equal_raw(data + uni64(out_off[i]) + done, data + uni64(out_off[r]) + done, plen);
    if (!eq && EH_LANE == 0) atomicOr(&flag[i], 1u);
  }
}
__global__ void __launch_bounds__(64) eh_uq_final_kernel(const uint64_t* out_len_, const int32_t* status_, uint64_t n, uint64_t* first_of_, const uint32_t* flag_,
                                                         unsigned long long* count_) {
  cqptr out_len = (cqptr)out_len_; const EH_G int32_t* status = (const EH_G int32_t*)status_; qptr first_of = (qptr)first_of_; cwptr flag = (cwptr)flag_;
  EH_G unsigned long long* count = (EH_G unsigned long long*)count_;
  for (uint64_t base = (uint64_t)blockIdx.x * 64; base < n; base += (uint64_t)gridDim.x * 64) {
    const uint64_t i = base + (uint64_t)EH_LANE;
    uint64_t uniq = 0, bytes = 0;
    if (i < n) {
      if (flag[i]) first_of[i] = i;                                  // differs from its key's first: reported unique (the collision rule of the header)
      if (status[i] == CASE_OK && first_of[i] == i) { uniq = 1; bytes = out_len[i]; }
    }
    uniq = uq_wave_add64(uniq); bytes = uq_wave_add64(bytes);
    if (EH_LANE == 0 && uniq) { atomicAdd(&count[0], (unsigned long long)uniq); atomicAdd(&count[1], (unsigned long long)bytes); }
  }
}

}  // namespace eh
