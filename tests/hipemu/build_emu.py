#!/usr/bin/env python3
"""Builds build/liberlamsa_hip_emu.so: the unmodified engine sources compiled with g++ against the CPU
stand-in for <hip/hip_runtime.h> in this directory.  TEST INFRASTRUCTURE (see hip/hip_runtime.h)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "build", "liberlamsa_hip_emu.so")


OUT_RACE = os.path.join(ROOT, "build", "liberlamsa_hip_emu_race.so")


def build(force=False, race=False):
    """race=True: the same sources with every load / store of the kernel code calling into race_hooks.cpp (see there)"""
    src = os.path.join(ROOT, "erlamsa_amd", "csrc")
    deps = [os.path.join(src, f) for f in os.listdir(src)] + [os.path.join(ROOT, "include", "erlamsa_hip.h"),
                                                                 os.path.join(ROOT, "tests", "hipemu", "hip", "hip_runtime.h")]
    out = OUT_RACE if race else OUT
    hooks = os.path.join(ROOT, "tests", "hipemu", "race_hooks.cpp")
    if race:
        deps.append(hooks)
    if not force and os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-attributes",
            "-I", os.path.join(ROOT, "tests", "hipemu"), "-I", os.path.join(ROOT, "include")]
    if not race:
        subprocess.check_call(base + ["-x", "c++", "-shared", os.path.join(src, "eh_engine.hip"), "-o", out])
        return out
    obj = [out + ".engine.o", out + ".hooks.o"]
    subprocess.check_call(base + ["-DHIPEMU_RACE=1", "-fsanitize=kernel-address", "--param", "asan-instrumentation-with-call-threshold=0",
                                  "--param", "asan-globals=0", "--param", "asan-stack=0", "-x", "c++", "-c", os.path.join(src, "eh_engine.hip"), "-o", obj[0]])
    subprocess.check_call(base + ["-c", hooks, "-o", obj[1]])
    subprocess.check_call(["g++", "-shared", "-rdynamic"] + obj + ["-o", out])
    for o in obj:                                   # (11 MB of objects would travel with every gpurun snapshot)
        os.remove(o)
    return out


def _build_host_program(name, force):
    """tests/hipemu/<name>.cpp and the engine as one stand-alone program under AddressSanitizer.  -O0: the run is tiny, and the
    engine compiles in a fraction of the time."""
    src = os.path.join(ROOT, "erlamsa_amd", "csrc")
    main = os.path.join(ROOT, "tests", "hipemu", name + ".cpp")
    out = os.path.join(ROOT, "build", name)
    deps = [os.path.join(src, f) for f in os.listdir(src)] + [os.path.join(ROOT, "include", "erlamsa_hip.h"),
                                                                 os.path.join(ROOT, "tests", "hipemu", "hip", "hip_runtime.h"), main]
    if not force and os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O0", "-g", "-std=c++17", "-ffp-contract=off", "-Wno-attributes", "-fsanitize=address", "-pthread",
                           "-I", os.path.join(ROOT, "tests", "hipemu"), "-I", os.path.join(ROOT, "include"),
                           main, "-x", "c++", os.path.join(src, "eh_engine.hip"), "-o", out])
    return out


def build_host_oom(force=False):
    """a context whose device allocations fail (see host_oom.cpp)"""
    return _build_host_program("host_oom", force)


def build_host_lifecycle(force=False):
    """two contexts that make, and release, every lazily created handle and buffer (see host_lifecycle.cpp)"""
    return _build_host_program("host_lifecycle", force)


OUT_COALESCE_UNIT = os.path.join(ROOT, "build", "coalesce_unit")


def build_coalesce_unit(force=False):
    """coalesce_unit.cpp and the coalescer's bookkeeping header, which needs neither HIP nor the emulator, as a stand-alone
    program under AddressSanitizer and UndefinedBehaviorSanitizer (see coalesce_unit.cpp)."""
    main = os.path.join(ROOT, "tests", "hipemu", "coalesce_unit.cpp")
    deps = [main, os.path.join(ROOT, "erlamsa_amd", "csrc", "eh_coalesce.h"), os.path.join(ROOT, "include", "erlamsa_hip.h")]
    if not force and os.path.exists(OUT_COALESCE_UNIT) and all(os.path.getmtime(d) <= os.path.getmtime(OUT_COALESCE_UNIT) for d in deps):
        return OUT_COALESCE_UNIT
    os.makedirs(os.path.dirname(OUT_COALESCE_UNIT), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", main, "-o", OUT_COALESCE_UNIT])
    return OUT_COALESCE_UNIT


if __name__ == "__main__":
    if "--coalesce-unit" in sys.argv:
        print(build_coalesce_unit(force="--force" in sys.argv))
    elif "--host-oom" in sys.argv:
        print(build_host_oom(force="--force" in sys.argv))
    elif "--host-lifecycle" in sys.argv:
        print(build_host_lifecycle(force="--force" in sys.argv))
    else:
        print(build(force="--force" in sys.argv, race="--race" in sys.argv))
