// The rule for GPU_MAX_HW_QUEUES at load time (erlamsa_amd/csrc/eh_host_queues.h) alone: no engine, no emulator, no HIP.
// TEST INFRASTRUCTURE: a stand-alone program, built by build_hw_queue_rule.py next to it with AddressSanitizer and
// UndefinedBehaviorSanitizer and run by tests/test_hw_queue_rule.py.  Every argument is one value of the variable ("-" alone: not
// set); one line "<argument> -> write N" or "<argument> -> leave" each.  Every value is handed over in a heap block of exactly its
// length + 1, so that a read past the terminator is a sanitizer report.
#include "../../erlamsa_amd/csrc/eh_host_queues.h"

#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++) {
    int w;
    if (!strcmp(argv[i], "-")) w = eh::hw_queues_to_write(nullptr);
    else {
      std::vector<char> exact(argv[i], argv[i] + strlen(argv[i]) + 1);
      w = eh::hw_queues_to_write(exact.data());
    }
    if (w) printf("%s -> write %d\n", argv[i], w); else printf("%s -> leave\n", argv[i]);
  }
  printf("hw_queue_rule ok\n");
  return 0;
}
