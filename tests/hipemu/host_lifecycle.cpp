// A context makes every handle and buffer that the host side creates lazily, is destroyed, and a second one does the same: both
// rounds give the same bytes, and nothing is left behind.
// TEST INFRASTRUCTURE: a stand-alone program, built by build_emu.build_host_lifecycle() from this file and the unmodified engine
// against the CPU stand-in for <hip/hip_runtime.h>, with AddressSanitizer and its leak check; tests/test_emulated_buffers.py runs
// it.  The stand-in's hipEventCreate and hipHostMalloc allocate host memory, so an event or a page-locked block that no part of the
// context releases is reported as a leak, and one released twice as a double free.  (Its streams are null handles: stream
// ownership is exercised on the device, tests/test_gpu_lifecycle.py.)  Exit status 0 and the line "host_lifecycle ok" mean that
// every step went as the comments say.
#include <erlamsa_hip.h>

#include <cstdio>
#include <cstring>
#include <vector>

#define STEP(cond)                                                                                \
  do {                                                                                            \
    if (!(cond)) { fprintf(stderr, "host_lifecycle: line %d: %s: %s\n", __LINE__, #cond, eh_last_error(ctx)); return 1; } \
  } while (0)

// everything a round reads back, in the order it reads it
struct Round {
  std::vector<uint8_t> bytes; std::vector<uint64_t> nums; std::vector<int32_t> status;
  bool operator==(const Round& o) const { return bytes == o.bytes && nums == o.nums && status == o.status; }
};

static int configure(eh_ctx* ctx, uint32_t flags) {
  eh_options o;
  memset(&o, 0, sizeof(o));
  o.abi_version = EH_ABI_VERSION;
  o.mutations = "bd,bf,bi"; o.patterns = "od,nd";
  o.max_case_bytes = 64 << 10; o.pool_bytes = 16 << 20; o.out_capacity = 1 << 20; o.flags = flags;
  return eh_configure(ctx, &o);
}

// a batch of 8 and its download (bytes, offsets, statuses)
static int batch(eh_ctx* ctx, void* stream, Round* r) {
  const int64_t seed[3] = {1, 2, 3};
  STEP(eh_fuzz_batch(ctx, seed, 1, 0, 8, stream) == EH_OK);
  uint64_t in_b = 0, out_b = 0, n = 0;
  STEP(eh_result_totals(ctx, &in_b, &out_b, &n) == EH_OK && n == 8);
  std::vector<uint8_t> data(out_b ? out_b : 1); std::vector<uint64_t> off(n + 1); std::vector<int32_t> st(n);
  STEP(eh_result_download(ctx, data.data(), data.size(), off.data(), st.data()) == EH_OK);
  STEP(off[n] == out_b && out_b > 0);
  r->bytes.insert(r->bytes.end(), data.begin(), data.begin() + out_b);
  r->nums.insert(r->nums.end(), off.begin(), off.end());
  r->status.insert(r->status.end(), st.begin(), st.end());
  return 0;
}

static int round_trip(Round* r) {
  eh_ctx* ctx = nullptr;
  STEP(eh_create(0, &ctx) == EH_OK);
  STEP(configure(ctx, EH_FLAG_META_TRACE) == EH_OK);
  std::vector<uint8_t> corpus(800);
  std::vector<uint64_t> coff(9);
  for (size_t i = 0; i < corpus.size(); i++) corpus[i] = (uint8_t)(i * 37 + (i >> 3));
  for (size_t i = 0; i <= 8; i++) coff[i] = 100 * i;
  STEP(eh_corpus_upload(ctx, corpus.data(), coff.data(), 8) == EH_OK);
  STEP(eh_reserve(ctx, 8) == EH_OK);
  if (batch(ctx, nullptr, r)) return 1;                                 // ... and eh_result_download: the gather streams, events and bounce buffers

  const uint64_t idx[3] = {7, 0, 3};
  uint64_t soff[4] = {0, 0, 0, 0};
  STEP(eh_result_download_select(ctx, idx, 3, nullptr, 0, soff) == EH_OK);
  std::vector<uint8_t> sel(soff[3] ? soff[3] : 1);
  STEP(eh_result_download_select(ctx, idx, 3, sel.data(), sel.size(), soff) == EH_OK);
  r->bytes.insert(r->bytes.end(), sel.begin(), sel.begin() + soff[3]);
  r->nums.insert(r->nums.end(), soff, soff + 4);

  uint64_t sum[9];
  STEP(eh_result_summary(ctx, sum) == EH_OK && sum[2] == 8);            // the page-locked totals
  r->nums.insert(r->nums.end(), sum, sum + 9);

  uint64_t first_of[8], n_unique = 0, unique_bytes = 0;
  STEP(eh_result_unique(ctx, first_of, &n_unique, &unique_bytes) == EH_OK);
  r->nums.insert(r->nums.end(), first_of, first_of + 8);
  r->nums.push_back(n_unique); r->nums.push_back(unique_bytes);

  uint8_t cls[8]; uint64_t n_fresh = 0, fresh_bytes = 0;
  STEP(eh_seen_reserve(ctx, 64) == EH_OK);
  STEP(eh_result_seen(ctx, 1, cls, &n_fresh, &fresh_bytes) == EH_OK);
  r->bytes.insert(r->bytes.end(), cls, cls + 8);
  r->nums.push_back(n_fresh); r->nums.push_back(fresh_bytes);

  void* stream = nullptr;
  STEP(eh_stream(ctx, &stream) == EH_OK);                               // the context's own stream

  uint64_t ticket[4];
  for (int k = 0; k < 4; k++) { const int64_t seed[3] = {5, 6, 7 + k}; STEP(eh_submit(ctx, corpus.data() + 100 * k, 100, seed, &ticket[k]) == EH_OK); }
  STEP(eh_flush(ctx) == EH_OK);
  for (int k = 0; k < 4; k++) {
    std::vector<uint8_t> out(64 << 10); uint64_t len = 0; int32_t st = -1;
    STEP(eh_poll(ctx, ticket[k], out.data(), out.size(), &len, &st) == EH_OK);
    r->bytes.insert(r->bytes.end(), out.begin(), out.begin() + len);
    r->nums.push_back(len); r->status.push_back(st);
  }

  // the second arena and the ordered offsets; the coalescer's batch replaced the corpus
  STEP(configure(ctx, EH_FLAG_ORDERED_OUTPUT) == EH_OK);
  STEP(eh_corpus_upload(ctx, corpus.data(), coff.data(), 8) == EH_OK);
  if (batch(ctx, stream, r)) return 1;
  eh_destroy(ctx);
  return 0;
}

int main() {
  Round first, second;
  if (round_trip(&first) || round_trip(&second)) return 1;
  if (!(first == second)) { fprintf(stderr, "host_lifecycle: the second context's results differ from the first's\n"); return 1; }
  printf("host_lifecycle ok\n");
  return 0;
}
