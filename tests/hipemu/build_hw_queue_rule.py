#!/usr/bin/env python3
"""Builds build/hw_queue_rule: hw_queue_rule.cpp and the rule for GPU_MAX_HW_QUEUES at load time (csrc/eh_host_queues.h), which needs
neither HIP nor the emulator, as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer - the pattern of
build_emu.build_coalesce_unit, with the same options.  TEST INFRASTRUCTURE (see hw_queue_rule.cpp)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "build", "hw_queue_rule")


def build(force=False):
    main = os.path.join(ROOT, "tests", "hipemu", "hw_queue_rule.cpp")
    deps = [main, os.path.join(ROOT, "erlamsa_amd", "csrc", "eh_host_queues.h")]
    if not force and os.path.exists(OUT) and all(os.path.getmtime(d) <= os.path.getmtime(OUT) for d in deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", main, "-o", OUT])
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
