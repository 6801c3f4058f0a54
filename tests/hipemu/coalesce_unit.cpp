// The request coalescer's bookkeeping (erlamsa_amd/csrc/eh_coalesce.h) alone, against a naive model: no engine, no emulator.
// TEST INFRASTRUCTURE: a stand-alone program, built by build_emu.build_coalesce_unit() with AddressSanitizer and
// UndefinedBehaviorSanitizer and run by tests/test_coalesce_unit.py.  Exit status 0 and the line "coalesce_unit ok" mean that
// every check held.
#include "../../erlamsa_amd/csrc/eh_coalesce.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace eh;

#define CHECK(cond)                                                                                  \
  do {                                                                                               \
    if (!(cond)) { fprintf(stderr, "coalesce_unit: line %d: %s\n", __LINE__, #cond); exit(1); }      \
  } while (0)

struct Req { uint64_t ticket; std::vector<uint8_t> bytes; int64_t seed[3]; uint32_t profile; };
typedef std::vector<Req> Model;

static Req make(uint64_t ticket, size_t len) {
  Req r; r.ticket = ticket; r.profile = (uint32_t)(ticket % 3);
  for (size_t i = 0; i < len; i++) r.bytes.push_back((uint8_t)(ticket * 131 + i * 7));
  for (int k = 0; k < 3; k++) r.seed[k] = (int64_t)(ticket * 10 + k);
  return r;
}
static bool push(CoBatch& b, const Req& r) { return b.push(r.ticket, r.bytes.data(), r.bytes.size(), r.seed, r.profile); }

// all five arrays of the batch are the model's requests packed in order
static void same(const CoBatch& b, const Model& m) {
  std::vector<uint8_t> data; std::vector<uint64_t> off{0}, tickets; std::vector<int64_t> seeds; std::vector<uint32_t> profile;
  bool any = false;
  for (const Req& r : m) {
    data.insert(data.end(), r.bytes.begin(), r.bytes.end()); off.push_back(data.size());
    seeds.insert(seeds.end(), r.seed, r.seed + 3); profile.push_back(r.profile); tickets.push_back(r.ticket);
    any = any || r.profile != 0;
  }
  CHECK(b.data == data); CHECK(b.off == off); CHECK(b.seeds == seeds); CHECK(b.profile == profile); CHECK(b.tickets == tickets);
  CHECK(b.off.front() == 0 && b.off.back() == b.data.size());
  CHECK(b.size() == m.size() && b.bytes() == data.size() && b.profiled() == any);
}

static void erase_each_position() {
  const size_t lens[4] = {0, 5, 0, 300};
  for (size_t gone = 0; gone < 4; gone++) {              // 0: empty at the start, 2: empty in the middle, 3: the last
    CoBatch b; Model m;
    for (size_t i = 0; i < 4; i++) { m.push_back(make(i + 1, lens[i])); CHECK(push(b, m.back())); }
    same(b, m);
    CHECK(b.erase(gone + 1)); m.erase(m.begin() + gone);
    same(b, m);
    CHECK(!b.erase(gone + 1));                          // (it has left)
    same(b, m);
  }
}

static void random_walk() {
  const size_t lens[6] = {0, 1, 15, 16, 17, 300};
  std::mt19937_64 rng(20250117);
  CoBatch b; Model m; uint64_t next = 1;
  for (int step = 0; step < 2000; step++) {
    if (m.empty() || rng() % 5 < 3) { m.push_back(make(next++, lens[rng() % 6])); CHECK(push(b, m.back())); }
    else { const size_t i = rng() % m.size(); CHECK(b.erase(m[i].ticket)); m.erase(m.begin() + i); }
    same(b, m);
  }
  CHECK(!b.erase(next));
  b.clear(); m.clear();
  same(b, m);
  CHECK(b.off.size() == 1);
}

static void flush_limits() {
  Coalescer c; c.flush_cases = 5; c.flush_bytes = 1 << 20;
  for (uint64_t t = 1; t <= 4; t++) CHECK(push(c.pending, make(t, 3)));
  CHECK(!c.at_limit());                                  // flush_cases - 1
  CHECK(push(c.pending, make(5, 3)));
  CHECK(c.at_limit());                                   // flush_cases
  Coalescer d; d.flush_cases = 100; d.flush_bytes = 317;
  CHECK(push(d.pending, make(1, 300))); CHECK(push(d.pending, make(2, 16)));
  CHECK(d.pending.bytes() == 316 && !d.at_limit());      // flush_bytes - 1
  CHECK(push(d.pending, make(3, 1)));
  CHECK(d.pending.bytes() == 317 && d.at_limit());       // flush_bytes
}

// six requests launched, two cancelled, one of the survivors with an empty output; -> the coalescer after "collected"
static void states_and_transitions() {
  Coalescer c;
  CHECK(c.next_ticket == 1 && !c.busy());
  CHECK(c.where(1) == CoWhere::unknown);
  for (uint64_t t = 1; t <= 6; t++) CHECK(push(c.pending, make(t, 4 * t)));
  CHECK(c.busy() && !c.in_flight);
  for (uint64_t t = 1; t <= 6; t++) CHECK(c.where(t) == CoWhere::pending);
  c.launched();
  CHECK(c.busy() && c.in_flight);
  CHECK(c.pending.size() == 0 && c.pending.bytes() == 0 && c.pending.off == std::vector<uint64_t>{0});
  CHECK(c.pending.seeds.empty() && c.pending.profile.empty());
  CHECK((c.flying == std::vector<uint64_t>{1, 2, 3, 4, 5, 6}));
  CHECK(push(c.pending, make(7, 2)));                   // the next batch fills while this one runs
  CHECK(c.where(3) == CoWhere::in_flight && c.where(7) == CoWhere::pending && c.where(8) == CoWhere::unknown);
  // cancel: in flight (twice), pending, unknown
  CHECK(c.cancel(2) == EH_OK && c.cancel(2) == EH_OK && c.cancel(5) == EH_OK);
  CHECK(c.where(2) == CoWhere::in_flight);              // (it leaves when the batch is collected)
  CHECK(c.cancel(7) == EH_OK && c.where(7) == CoWhere::unknown && c.pending.size() == 0 && c.pending.off == std::vector<uint64_t>{0});
  CHECK(c.cancel(7) == EH_E_INVALID && c.cancel(99) == EH_E_INVALID);
  CHECK(c.busy());                                      // (the batch in flight)
  // the results: ticket t gets t - 1 bytes of value t (ticket 1: none) and status t % 2
  const std::vector<uint64_t> tickets = c.flying;
  std::vector<uint8_t> data; std::vector<uint64_t> off{0}; std::vector<int32_t> st;
  for (uint64_t t = 1; t <= 6; t++) { data.insert(data.end(), t - 1, (uint8_t)t); off.push_back(data.size()); st.push_back((int32_t)(t % 2)); }
  c.collected(tickets, data.data(), off.data(), st.data());
  CHECK(!c.in_flight && c.flying.empty() && c.cancelled.empty() && !c.busy());
  CHECK(c.where(2) == CoWhere::unknown && c.where(5) == CoWhere::unknown && c.done.size() == 4);
  for (uint64_t t : {1, 3, 4, 6}) {
    CHECK(c.where(t) == CoWhere::done);
    CHECK(c.done.at(t).out == std::vector<uint8_t>(t - 1, (uint8_t)t) && c.done.at(t).status == (int32_t)(t % 2));
  }
  // cancel: done, then the same ticket again
  CHECK(c.cancel(3) == EH_OK && c.where(3) == CoWhere::unknown && c.cancel(3) == EH_E_INVALID);
  CHECK(c.cancel(2) == EH_E_INVALID);                   // (was cancelled in flight: gone with the batch)
  CHECK(c.done.size() == 3);
}

int main() {
  erase_each_position();
  random_walk();
  flush_limits();
  states_and_transitions();
  printf("coalesce_unit ok\n");
  return 0;
}
