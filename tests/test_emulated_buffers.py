"""The device buffers and handles of the engine's host side (csrc/eh_host.h: DevBuf and the parts of a context) without a GPU: a
context whose allocations fail, and two contexts that make and release everything that is created lazily, as stand-alone programs
under AddressSanitizer (tests/hipemu/host_oom.cpp, host_lifecycle.cpp), and a context whose buffers grow and are reused, on the CPU
wavefront emulator against the oracle (tests/hipemu/emu_buffers.py; tests/test_gpu_buffers.py runs the same body on the gfx950
binary)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))


def test_context_survives_failed_allocations():
    """a batch of 8, eh_reserve(2^45) fails, the same batch again; an arena of 2^48 bytes fails, the same batch again; eh_destroy:
    no report from AddressSanitizer (allocator_may_return_null: the oversized requests fail instead of ending the program)"""
    import build_emu
    exe = build_emu.build_host_oom()
    env = dict(os.environ, ASAN_OPTIONS="allocator_may_return_null=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.splitlines()[-1] == "host_oom ok", r.stdout[-2000:]


def test_contexts_release_what_they_made():
    """twice in one process, on a fresh context each: every call that makes a handle or a buffer on first use (downloads, summary,
    filter, seen set, own stream, coalescer, ordered output), then eh_destroy.  Equal results, no report from AddressSanitizer, and
    none from its leak check: the emulator's events and page-locked blocks are host allocations.  (Where the leak check cannot
    attach to its own process it says so and is switched off; use after free and double free are still reported.)"""
    import build_emu
    exe = build_emu.build_host_lifecycle()
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=300)
    if "LeakSanitizer has encountered a fatal error" in r.stderr:
        r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.splitlines()[-1] == "host_lifecycle ok", r.stdout[-2000:]


def test_emulated_buffers_grow_and_are_reused():
    """n = 8, 200, 200 ordered twice, 8, fuzz_calls 16 and 300 profiled, a corpus three times as large and the small one again, on
    one context: every download, digest, first_of and selective download equals the oracle's"""
    import build_emu
    env = dict(os.environ, ERLAMSA_HIP_LIB=build_emu.build())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hipemu", "emu_buffers.py")], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.splitlines()[-1:] == ["buffers ok"], r.stdout[-2000:] + r.stderr[-2000:]
