// A context must stay usable, and destroy cleanly, after a device allocation of the engine's host side has failed.
// TEST INFRASTRUCTURE: a stand-alone program, built by build_emu.build_host_oom() from this file and the unmodified engine
// against the CPU stand-in for <hip/hip_runtime.h>, with AddressSanitizer; tests/test_emulated_buffers.py runs it with
// ASAN_OPTIONS=allocator_may_return_null=1 (the oversized requests below come back as out-of-memory instead of ending the
// program).  Exit status 0 and the line "host_oom ok" mean that every step went as the comments say.
#include <erlamsa_hip.h>

#include <cstdio>
#include <cstring>
#include <vector>

#define STEP(cond)                                                                                \
  do {                                                                                            \
    if (!(cond)) { fprintf(stderr, "host_oom: line %d: %s: %s\n", __LINE__, #cond, eh_last_error(ctx)); return 1; } \
  } while (0)

static eh_ctx* ctx = nullptr;

static int configure(uint64_t out_capacity) {
  eh_options o;
  memset(&o, 0, sizeof(o));
  o.abi_version = EH_ABI_VERSION;
  o.mutations = "bd,bf,bi"; o.patterns = "od,nd";
  o.max_case_bytes = 64 << 10; o.pool_bytes = 16 << 20; o.out_capacity = out_capacity;
  return eh_configure(ctx, &o);
}

struct Result { std::vector<uint8_t> data; std::vector<uint64_t> off; std::vector<int32_t> status; };
static bool operator==(const Result& a, const Result& b) { return a.data == b.data && a.off == b.off && a.status == b.status; }

static int batch(Result* r) {
  const int64_t seed[3] = {1, 2, 3};
  int rc = eh_fuzz_batch(ctx, seed, 1, 0, 8, nullptr);
  if (rc) return rc;
  uint64_t in_b = 0, out_b = 0, n = 0;
  rc = eh_result_totals(ctx, &in_b, &out_b, &n);
  if (rc) return rc;
  if (n != 8) return -100;
  r->data.assign(out_b ? out_b : 1, 0); r->off.assign(n + 1, 0); r->status.assign(n, -1);
  rc = eh_result_download(ctx, r->data.data(), r->data.size(), r->off.data(), r->status.data());
  r->data.resize(out_b);
  return rc;
}

int main() {
  STEP(eh_create(0, &ctx) == EH_OK);
  STEP(configure(1 << 20) == EH_OK);
  std::vector<uint8_t> corpus(800);
  std::vector<uint64_t> off(9);
  for (size_t i = 0; i < corpus.size(); i++) corpus[i] = (uint8_t)(i * 37 + (i >> 3));
  for (size_t i = 0; i <= 8; i++) off[i] = 100 * i;
  STEP(eh_corpus_upload(ctx, corpus.data(), off.data(), 8) == EH_OK);
  Result first, again;
  STEP(batch(&first) == EH_OK);
  STEP(first.off[8] > 0);

  // the result arrays cannot grow to 2^45 cases: the next batch of 8 gets arrays of its size again
  STEP(eh_reserve(ctx, 1ull << 45) != EH_OK);
  STEP(batch(&again) == EH_OK);
  STEP(again == first);

  // an output arena that cannot be had: the batch fails, and the next configuration gets its arena
  STEP(configure(1ull << 48) == EH_OK);
  STEP(batch(&again) != EH_OK);
  STEP(configure(1 << 20) == EH_OK);
  STEP(batch(&again) == EH_OK);
  STEP(again == first);

  eh_destroy(ctx);
  printf("host_oom ok\n");
  return 0;
}
