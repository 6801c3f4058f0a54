// eh_seen.h — the seen set: the keys (length, digest) of outputs of EARLIER batches, kept in device memory, so that a batch's results
// are told from them where they lie (include/erlamsa_hip.h: eh_seen_reserve .. eh_result_seen, eh_selftest_seen).
//
// What it stands for on the reference side: radamsa's --checksums N, the checksum set it keeps over a whole run.  The uniqueness
// filter (eh_unique.h) finds the repeats inside one batch and forgets; this is the part that persists.
//
//   keys[2 capacity]   the key log, append-only: pair k = {length, digest} of the k-th key ever recorded (the export order)
//   tab[slots]         open addressing, slots = the power of two >= 2 capacity: a word is an index into the log or SN_EMPTY.  A
//                      key is read THROUGH the word, as the filter reads it through its owner, so every 64-bit value is a legal
//                      digest and no key word is ever a marker
//   ctr[4]             [0] keys held, [1] keys dropped because the log was full, [2] fresh cases and [3] their bytes of the last call
//
// A batch has been through the filter first: first_of and the mismatch flags say which cases are the first of their bytes, and
// those alone are looked up.  Launches, all on the context's stream, none waits for another workgroup:
//   eh_sn_lookup_kernel   cls[i]: 3 not EH_CASE_OK, 1 a repeat inside the batch, 2 its key is in the set, 0 fresh   (the table is only read)
//   eh_sn_rank_kernel     pos[i] = held + the fresh, unflagged cases in front of case i, SN_EMPTY from `capacity` on   (one wavefront, like eh_uq_scan_kernel)
//   eh_sn_append_kernel   keys[pos[i]] = case i's key                                                              (plain stores)
//   eh_sn_insert_kernel   one lane per appended key: atomicCAS(SN_EMPTY -> pos[i]) on the first free word of its probe chain
// Log positions come from a scan over the case index, so the log, and with it the export, never depends on scheduling; which WORD
// of the table a key ends up in does, and nothing reads that.
#pragma once
#include "eh_unique.h"

namespace eh {

constexpr unsigned long long SN_EMPTY = ~0ull;

// the lengths of the corpus entries, for the filter's kernels to run over the corpus arena (eh_seen_add_corpus)
__global__ void __launch_bounds__(64) eh_sn_lens_kernel(const uint64_t* off_, uint64_t* len_, uint64_t n) {
  cqptr off = (cqptr)off_; qptr len = (qptr)len_;
  for (uint64_t i = (uint64_t)blockIdx.x * 64 + (uint64_t)EH_LANE; i < n; i += (uint64_t)gridDim.x * 64) len[i] = off[i + 1] - off[i];
}

// status_ / first_of_ may be null: every case EH_CASE_OK / its own first (keys from outside, which have no bytes to compare)
__global__ void __launch_bounds__(64) eh_sn_lookup_kernel(const uint64_t* len_, const int32_t* status_, const uint64_t* digest_, const uint64_t* first_of_, uint64_t n,
                                                          const uint64_t* keys_, const unsigned long long* tab_, uint64_t slots, uint8_t* cls_) {
  cqptr len = (cqptr)len_, digest = (cqptr)digest_, first_of = (cqptr)first_of_, keys = (cqptr)keys_; const EH_G int32_t* status = (const EH_G int32_t*)status_;
  const EH_G unsigned long long* tab = (const EH_G unsigned long long*)tab_; bptr cls = (bptr)cls_;
  for (uint64_t i = (uint64_t)blockIdx.x * 64 + (uint64_t)EH_LANE; i < n; i += (uint64_t)gridDim.x * 64) {
    uint8_t c = 0;
    if (status && status[i] != CASE_OK) c = 3;
    else if (first_of && first_of[i] != i) c = 1;
    else {
      const uint64_t ln = len[i], dig = digest[i];
      uint64_t s = uq_hash(ln, dig) & (slots - 1);
      for (uint64_t tries = 0; tries < slots; tries++, s = (s + 1) & (slots - 1)) {      // (at most capacity of the >= 2 capacity words are ever taken)
        const unsigned long long w = tab[s];
        if (w == SN_EMPTY) break;
        if (keys[2 * w] == ln && keys[2 * w + 1] == dig) { c = 2; break; }
      }
    }
    cls[i] = c;
  }
}

// One wavefront, 64 cases per step.  Counts the fresh cases and their bytes; with `commit`, numbers those of them that carry a key
// of their own (flag_ may be null: all do) from the log's end on, in case order, and moves the counters.
__global__ void __launch_bounds__(64) eh_sn_rank_kernel(const uint64_t* len_, const uint8_t* cls_, const uint32_t* flag_, uint64_t n, uint64_t capacity, uint32_t commit,
                                                        unsigned long long* ctr_, uint64_t* pos_) {
  cqptr len = (cqptr)len_; cbptr cls = (cbptr)cls_; cwptr flag = (cwptr)flag_; qptr pos = (qptr)pos_;
  EH_G unsigned long long* ctr = (EH_G unsigned long long*)ctr_;
  const int l = EH_LANE;
  const uint64_t held = uni64(ctr[0]);
  uint64_t run = 0, fresh = 0, bytes = 0;
  for (uint64_t base = 0; base < n; base += 64) {
    const uint64_t i = base + (uint64_t)l;
    const bool f = i < n && cls[i] == 0;
    if (f) { fresh++; bytes += len[i]; }
    if (!commit) continue;
    const bool r = f && !(flag && flag[i]);
    const unsigned long long m = __ballot(r);
    const uint64_t p = held + run + (uint64_t)__popcll(m & ((1ull << l) - 1));
    if (i < n) pos[i] = r && p < capacity ? p : SN_EMPTY;
    run += (uint64_t)__popcll(m);
  }
  fresh = uq_wave_add64(fresh); bytes = uq_wave_add64(bytes);
  if (l == 0) {
    ctr[2] = fresh; ctr[3] = bytes;
    if (commit) {
      const uint64_t all = held + run, kept = all < capacity ? all : capacity;
      ctr[0] = kept; ctr[1] += all - kept;
    }
  }
}

__global__ void __launch_bounds__(64) eh_sn_append_kernel(const uint64_t* len_, const uint64_t* digest_, const uint64_t* pos_, uint64_t n, uint64_t* keys_) {
  cqptr len = (cqptr)len_, digest = (cqptr)digest_, pos = (cqptr)pos_; qptr keys = (qptr)keys_;
  for (uint64_t i = (uint64_t)blockIdx.x * 64 + (uint64_t)EH_LANE; i < n; i += (uint64_t)gridDim.x * 64) {
    const uint64_t p = pos[i];
    if (p == SN_EMPTY) continue;
    keys[2 * p] = len[i]; keys[2 * p + 1] = digest[i];
  }
}

// Every key the words can point to is complete: this batch's were stored by the kernel before, the others by earlier batches.  A
// lane that loses a word to another lane reads that lane's key through it and probes on; nobody waits.
__global__ void __launch_bounds__(64) eh_sn_insert_kernel(const uint64_t* pos_, uint64_t n, const uint64_t* keys_, unsigned long long* tab_, uint64_t slots) {
  cqptr pos = (cqptr)pos_, keys = (cqptr)keys_; EH_G unsigned long long* tab = (EH_G unsigned long long*)tab_;
  for (uint64_t i = (uint64_t)blockIdx.x * 64 + (uint64_t)EH_LANE; i < n; i += (uint64_t)gridDim.x * 64) {
    const uint64_t p = pos[i];
    if (p == SN_EMPTY) continue;
    const uint64_t ln = keys[2 * p], dig = keys[2 * p + 1];
    uint64_t s = uq_hash(ln, dig) & (slots - 1);
    for (uint64_t tries = 0; tries < slots; tries++, s = (s + 1) & (slots - 1)) {
      unsigned long long w = tab[s];
      if (w == SN_EMPTY) { w = atomicCAS(&tab[s], SN_EMPTY, (unsigned long long)p); if (w == SN_EMPTY) break; }
      if (keys[2 * w] == ln && keys[2 * w + 1] == dig) break;          // (the ranked keys of a call are distinct and absent: not reached)
    }
  }
}

}  // namespace eh
