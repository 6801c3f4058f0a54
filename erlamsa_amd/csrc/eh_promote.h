// eh_promote.h — corpus promotion: outputs of the last batch become entries of the corpus arena, on the device
// (include/erlamsa_hip.h: eh_corpus_promote, eh_corpus_promote_fresh, eh_corpus_download, eh_selftest_promote).
//
// What it stands for on the reference side: the feedback loop around a radamsa-style mutator - take seeds, make cases, keep the new
// ones, mutate those.  The filter (eh_unique.h) and the seen set (eh_seen.h) say which outputs are worth keeping; this writes them
// where the next batch reads its seeds, and no kept byte crosses PCIe.
//
// The promoted entries are described by three m-entry arrays - where each lies in the source arena, its length, where it goes behind
// the destination's base - which the host builds for an explicit list and eh_pm_scan_kernel builds for the fresh cases.  From there
// on both entry points are the same code.  Launches, all on one stream, a workgroup is one wavefront, none waits for another workgroup:
//   eh_pm_select_kernel    elen[i] = the case's length if it is eligible, else 0                      (a lane per case)
//   eh_pm_scan_kernel      the budget rule over the inclusive sums of elen in case order; rank and destination of every taken
//                          case, compaction into the entry arrays, the two counters                  (one wavefront, like eh_sn_rank_kernel)
//   eh_pm_offsets_kernel   off[base_n + k] = base_bytes + dst[k], and the closing off[base_n + m]
//   eh_uq_scan_kernel      (eh_unique.h) piece_first over the m entry lengths
//   eh_pm_copy_kernel      wavefronts take piece numbers grid-stride, find the piece's entry by binary search and copy its up to
//                          UQ_PIECE bytes with wave_copy_raw: destinations are packed back to back, so they are at arbitrary byte
//                          addresses, and neighbouring pieces write disjoint bytes
// Work is cut by BYTES as in the filter (eh_unique.h "pieces, not cases"): an entry of 1 GiB is 16 384 pieces on as many wavefronts.
#pragma once
#include "eh_unique.h"

namespace eh {

// cls_ may be null (every EH_CASE_OK case is a candidate); max_entry 0: no limit.  Eligible: EH_CASE_OK, class 0, 1 <= len <= max_entry.
__global__ void __launch_bounds__(64) eh_pm_select_kernel(const int32_t* status_, const uint8_t* cls_, const uint64_t* len_, uint64_t n, uint64_t max_entry, uint64_t* elen_) {
  const EH_G int32_t* status = (const EH_G int32_t*)status_; cbptr cls = (cbptr)cls_; cqptr len = (cqptr)len_; qptr elen = (qptr)elen_;
  for (uint64_t i = (uint64_t)blockIdx.x * 64 + (uint64_t)EH_LANE; i < n; i += (uint64_t)gridDim.x * 64) {
    const uint64_t v = len[i];
    const bool ok = status[i] == CASE_OK && (!cls || cls[i] == 0) && v >= 1 && (!max_entry || v <= max_entry);
    elen[i] = ok ? v : 0;
  }
}

// One wavefront, 64 cases per step.  S(i) = inclusive sum of elen in case order; case i is taken iff elen[i] > 0 and S(i) <= max_total
// (0: no limit): the taken cases are a prefix of the eligible ones, so a taken case's destination is S(i) - elen[i].  Entry k of the
// compacted arrays is the k-th taken case; ctr[0] = taken cases, ctr[1] = their bytes.
__global__ void __launch_bounds__(64) eh_pm_scan_kernel(const uint64_t* elen_, const uint64_t* src_off_, uint64_t n, uint64_t max_total, unsigned long long* ctr_,
                                                        uint64_t* ent_src_, uint64_t* ent_len_, uint64_t* ent_dst_) {
  cqptr elen = (cqptr)elen_, src_off = (cqptr)src_off_; qptr ent_src = (qptr)ent_src_, ent_len = (qptr)ent_len_, ent_dst = (qptr)ent_dst_;
  EH_G unsigned long long* ctr = (EH_G unsigned long long*)ctr_;
  const int l = EH_LANE;
  uint64_t run = 0, taken = 0, bytes = 0;
  for (uint64_t base = 0; base < n; base += 64) {
    const uint64_t i = base + (uint64_t)l;
    const uint64_t v = i < n ? elen[i] : 0;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      uint64_t t = ((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(inc >> 32), d) << 32) | (uint32_t)__shfl_up((int)(uint32_t)inc, d);
      if (l >= d) inc += t;
    }
    const uint64_t s = run + inc;
    const bool take = v > 0 && (!max_total || s <= max_total);
    const unsigned long long m = __ballot(take);
    if (take) {
      const uint64_t k = taken + (uint64_t)__popcll(m & ((1ull << l) - 1));
      ent_src[k] = src_off[i]; ent_len[k] = v; ent_dst[k] = s - v;
      bytes += v;
    }
    taken += (uint64_t)__popcll(m);
    run += uni64(((uint64_t)(uint32_t)__shfl((int)(uint32_t)(inc >> 32), 63) << 32) | (uint32_t)__shfl((int)(uint32_t)inc, 63));
  }
  bytes = uq_wave_add64(bytes);
  if (l == 0) { ctr[0] = taken; ctr[1] = bytes; }
}

// the offsets of the m new entries behind the base_n the corpus keeps, and the closing offset
__global__ void __launch_bounds__(64) eh_pm_offsets_kernel(const uint64_t* ent_dst_, uint64_t m, uint64_t base_n, uint64_t base_bytes, uint64_t total, uint64_t* off_) {
  cqptr ent_dst = (cqptr)ent_dst_; qptr off = (qptr)off_;
  for (uint64_t k = (uint64_t)blockIdx.x * 64 + (uint64_t)EH_LANE; k <= m; k += (uint64_t)gridDim.x * 64) off[base_n + k] = base_bytes + (k < m ? ent_dst[k] : total);
}

// dst[ent_dst[k] ..) = src[ent_src[k] .. + ent_len[k]), piece by piece (piece_first: eh_uq_scan_kernel over ent_len)
__global__ void __launch_bounds__(64) eh_pm_copy_kernel(const uint8_t* src_, uint8_t* dst_, const uint64_t* ent_src_, const uint64_t* ent_len_, const uint64_t* ent_dst_,
                                                        const uint64_t* piece_first_, uint64_t m) {
  cbptr src = (cbptr)src_; bptr dst = (bptr)dst_; cqptr ent_src = (cqptr)ent_src_, ent_len = (cqptr)ent_len_, ent_dst = (cqptr)ent_dst_, piece_first = (cqptr)piece_first_;
  const uint64_t np = uni64(piece_first[m]);
  for (uint64_t p = blockIdx.x; p < np; p += gridDim.x) {
    const uint64_t k = uni64(uq_case_of(piece_first, m, p));
    const uint64_t len = uni64(ent_len[k]), done = (p - uni64(piece_first[k])) * UQ_PIECE;
    if (done >= len) continue;                                         // (cannot be: the entry has ceil(len / UQ_PIECE) pieces)
    const uint32_t plen = len - done > UQ_PIECE ? UQ_PIECE : (uint32_t)(len - done);
    wave_copy_raw(dst + uni64(ent_dst[k]) + done, src + uni64(ent_src[k]) + done, plen);
  }
}

}  // namespace eh
