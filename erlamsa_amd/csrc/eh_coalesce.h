// eh_coalesce.h — the bookkeeping of the request coalescer (eh_submit / eh_flush / eh_poll / eh_cancel), host side, no HIP, no eh_ctx:
// which requests wait for a launch, which tickets are on the device, which results wait to be polled.  The context (eh_host.h) keeps
// one Coalescer behind a std::mutex, and eh_host_coalesce.h does the launches and downloads; tests/hipemu/coalesce_unit.cpp checks this file alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <new>
#include <vector>

#include "../../include/erlamsa_hip.h"

namespace eh {

// The requests not launched yet, packed as eh_corpus_upload and eh_fuzz_calls_profiled take them: request i is data[off[i] .. off[i + 1])
// with seeds[3i .. 3i + 3), profile[i] and tickets[i].  off.front() == 0 and off.back() == data.size() at all times.
struct CoBatch {
  std::vector<uint8_t> data; std::vector<uint64_t> off{0}; std::vector<int64_t> seeds; std::vector<uint32_t> profile; std::vector<uint64_t> tickets;
  size_t size() const { return tickets.size(); }
  uint64_t bytes() const { return data.size(); }
  bool profiled() const { return std::any_of(profile.begin(), profile.end(), [](uint32_t id) { return id != 0; }); }
  // room for `extra` more elements (at least doubling, as push_back grows); throws what reserve throws
  template <class V> static void room(V& v, size_t extra) { if (v.capacity() - v.size() < extra) v.reserve(v.size() + std::max(extra, v.size())); }
  // appends the request to all five arrays or, out of memory (false), leaves all five as they were
  bool push(uint64_t ticket, const uint8_t* d, uint64_t len, const int64_t seed[3], uint32_t prof) {
    try { room(data, len); room(off, 1); room(seeds, 3); room(profile, 1); room(tickets, 1); } catch (const std::bad_alloc&) { return false; }
    if (len) data.insert(data.end(), d, d + len);                     // (there is room for all of it: nothing from here on throws)
    off.push_back(data.size()); seeds.insert(seeds.end(), seed, seed + 3); profile.push_back(prof); tickets.push_back(ticket);
    return true;
  }
  // the request leaves and the later ones move down by its length; false: no such ticket here
  bool erase(uint64_t ticket) {
    const size_t i = std::find(tickets.begin(), tickets.end(), ticket) - tickets.begin();
    if (i == tickets.size()) return false;
    const uint64_t a = off[i], b = off[i + 1];
    data.erase(data.begin() + a, data.begin() + b); off.erase(off.begin() + i + 1);
    for (size_t k = i + 1; k < off.size(); k++) off[k] -= b - a;
    seeds.erase(seeds.begin() + 3 * i, seeds.begin() + 3 * i + 3); profile.erase(profile.begin() + i); tickets.erase(tickets.begin() + i);
    return true;
  }
  void clear() { data.clear(); off.assign(1, 0); seeds.clear(); profile.clear(); tickets.clear(); }
};

struct CoResult { std::vector<uint8_t> out; int32_t status; };
enum class CoWhere { unknown, pending, in_flight, done };

// A ticket is in one place: pending (queued), in flight (launched, results on the device: one batch at most), done (downloaded, not
// polled yet), or nowhere (never given out, polled, cancelled).
struct Coalescer {
  CoBatch pending;
  bool in_flight = false; std::vector<uint64_t> flying;             // the launched batch's tickets, in submission order
  std::vector<uint64_t> cancelled;                                  // in-flight tickets nobody will poll
  std::map<uint64_t, CoResult> done;
  uint64_t next_ticket = 1, flush_cases = 4096, flush_bytes = 64ull << 20;
  static bool has(const std::vector<uint64_t>& v, uint64_t t) { return std::find(v.begin(), v.end(), t) != v.end(); }
  CoWhere where(uint64_t t) const {
    return done.count(t) ? CoWhere::done : has(pending.tickets, t) ? CoWhere::pending : has(flying, t) ? CoWhere::in_flight : CoWhere::unknown;
  }
  bool at_limit() const { return pending.size() >= flush_cases || pending.bytes() >= flush_bytes; }   // time to launch
  bool busy() const { return in_flight || pending.size() != 0; }    // the context's buffers and options are the coalescer's
  void launched() { in_flight = true; flying.swap(pending.tickets); pending.clear(); }
  // The in-flight batch is on the host: result i (data[off[i] .. off[i + 1]), status[i]) is filed under tickets[i], the caller's copy
  // of `flying` from before it released the lock, unless that ticket was cancelled meanwhile.
  void collected(const std::vector<uint64_t>& tickets, const uint8_t* data, const uint64_t* off, const int32_t* status) {
    for (size_t i = 0; i < tickets.size(); i++)
      if (!has(cancelled, tickets[i])) done.emplace(tickets[i], CoResult{std::vector<uint8_t>(data + off[i], data + off[i + 1]), status[i]});
    cancelled.clear(); in_flight = false; flying.clear();
  }
  // eh_cancel: a finished result is dropped, a pending request leaves its batch, an in-flight one is dropped when its batch is
  // collected (asking twice is fine); EH_E_INVALID for a ticket that is nowhere
  int cancel(uint64_t t) {
    const CoWhere w = where(t);
    if (w == CoWhere::done) done.erase(t); else if (w == CoWhere::pending) pending.erase(t); else if (w == CoWhere::in_flight) cancelled.push_back(t);
    return w == CoWhere::unknown ? EH_E_INVALID : EH_OK;
  }
};

}  // namespace eh
