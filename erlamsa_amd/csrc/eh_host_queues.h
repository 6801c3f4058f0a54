// eh_host_queues.h - how many hardware queues the library asks the HIP runtime for when it is loaded: the rule alone, host side,
// no HIP, no eh_ctx, nothing read or written but its argument.  eh_runtime_defaults (eh_engine.hip) applies it to GPU_MAX_HW_QUEUES;
// tests/hipemu/hw_queue_rule.cpp checks this file alone.
#pragma once

namespace eh {

// Passes in flight run on one HIP stream each and only run side by side when every stream has a hardware queue of its own.  Seven
// passes are what a device holds, and 8 / 12 / 16 queues measured the same (profiles/r06_wave_slots.txt): eight.
enum { EH_HW_QUEUES = 8 };

// `set` = what getenv("GPU_MAX_HW_QUEUES") gave (nullptr: not set).  -> the value to write, or 0: leave the variable as it is.
//   not set                           -> EH_HW_QUEUES
//   a plain decimal number below it   -> EH_HW_QUEUES (the runtime's default of 4, written out by whoever started the process, is
//                                        no choice of the host's: seven streams on four queues run in two shifts)
//   EH_HW_QUEUES or more              -> 0: never lowered, and nothing above EH_HW_QUEUES is ever written
//   anything else                     -> 0: "", a sign, a blank, trailing text, "0x4" - whatever the runtime makes of it is the host's
// Strict on purpose: every character must be a digit, so no strtol, no locale and no overflow - a number of any length is compared
// digit by digit (leading zeros dropped: "007" is 7).
static inline int hw_queues_to_write(const char* set) {
  if (!set) return EH_HW_QUEUES;
  if (!*set) return 0;
  const char* p = set;
  while (*p == '0') p++;
  const char* first = p;
  for (; *p; p++) if (*p < '0' || *p > '9') return 0;
  static_assert(EH_HW_QUEUES <= 10, "one significant digit decides");
  if (p - first > 1) return 0;                              // two significant digits or more: at least 10
  const int v = p == first ? 0 : *first - '0';
  return v < EH_HW_QUEUES ? EH_HW_QUEUES : 0;
}

}  // namespace eh
