"""Passes in flight overlap when the process starts with GPU_MAX_HW_QUEUES=4 (csrc/eh_host_queues.h, eh_runtime_defaults): the
library raises a preset 4 to 8 when it is loaded, before its first HIP call, so six streams get six hardware queues.  The effect
itself at the smallest shape that shows it: six contexts of ONE workgroup each (max_slots=1) hold six of the device's 2 048 wave
slots, so six identical passes contend for nothing but queues.  Run as a program (`python test_gpu_hw_queues.py N`) this file is
the child process that does the GPU work and prints one JSON line."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONTEXTS = 6
ROW = 256
N = 16384           # cases of a pass: sized once so that a lone pass lasts 0.2 - 0.5 s on the device (see the test's docstring)
SEED = (1, 2, 3)


def child(n):
    sys.path.insert(0, ROOT)
    import ctypes
    import hashlib
    import numpy as np
    import erlamsa_amd as ea
    ea.load_library()
    libc = ctypes.CDLL(None)
    libc.getenv.restype = ctypes.c_char_p
    after_load = libc.getenv(b"GPU_MAX_HW_QUEUES")                      # (os.environ is a snapshot)
    data = np.random.Generator(np.random.PCG64(0xE71A)).integers(0, 256, size=n * ROW, dtype=np.uint8)
    off = np.arange(n + 1, dtype=np.uint64) * ROW
    engines = []
    for _ in range(CONTEXTS):
        e = ea.Engine(0)
        e.configure(mutations="bd,bf,bi", patterns="od", max_slots=1, max_case_bytes=1 << 20, pool_bytes=256 << 20,
                    out_capacity=2 * n * ROW + (16 << 20))
        engines.append(e)
    engines[0].upload_corpus(data, off)
    for e in engines[1:]:
        e.share_corpus(engines[0])
    streams = [e.own_stream() for e in engines]
    for e, st in zip(engines, streams):                                   # device memory of a full pass, then the stream's first
        e.reserve(n)                                                      # dispatch (the runtime allocates the queue's scratch):
        e.fuzz_batch(seed=SEED, first_case=1, corpus_first=0, n=min(n, 64), stream=st)   # untimed, one context at a time
        e.sync()

    def timed(which):
        t0 = time.perf_counter()
        for k in which:
            engines[k].fuzz_batch(seed=SEED, first_case=1, corpus_first=0, n=n, stream=streams[k])
        for k in which:
            engines[k].sync()
        return time.perf_counter() - t0

    lone = [timed([0]), timed([0])]                                       # the first is also the full-size warm-up of the kernel
    t6 = timed(range(CONTEXTS))
    digests, arena_full = [], 0
    for e in engines:
        outs, status = e.download()
        arena_full += int((status == 4).sum())
        digests.append(hashlib.sha1(status.tobytes() + b"".join(len(o).to_bytes(8, "little") + o for o in outs)).hexdigest())
    kernel_ms = [round(e.kernel_ms(), 3) for e in engines]
    for e in reversed(engines):
        e.close()
    print(json.dumps({"n": n, "after_load": None if after_load is None else after_load.decode(), "lone_s": lone, "t1": min(lone), "t6": t6,
                      "ratio": t6 / min(lone), "kernel_ms_of_the_six": kernel_ms, "digests": digests, "arena_full": arena_full}), flush=True)


@pytest.mark.gpu
def test_six_passes_overlap_when_four_queues_are_preset():
    """One fresh child process started with GPU_MAX_HW_QUEUES=4: six contexts with max_slots=1, mutators bd,bf,bi, pattern od, a
    uniform corpus of N rows of 256 bytes, every context runs case numbers 1..N.  After one small untimed pass per context:
    t1 = a lone pass on context 0 (the faster of two, so the bound is the stricter one), t6 = all six launched back to back, then
    synchronised.  Six queues give t6 / t1 of about 1.0, six streams on four queues put two passes behind two others and give about
    2.0; asserted: t6 < 1.5 t1, the variable reads 8 after the load, and the six outputs are byte-identical.
    N = 16 384, sized once on an MI355X: a lone pass 0.254 s (4 096 cases: 0.063 s), the six together 0.266 s, t6 / t1 = 1.05.  The same
    child on the library before the rule (the variable stays 4): lone 0.263 s, the six 0.533 s, t6 / t1 = 2.03."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(N)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print("n %d: t1 %.4f s (lone passes %s), t6 %.4f s, t6 / t1 %.3f, GPU_MAX_HW_QUEUES after load %r"
          % (got["n"], got["t1"], got["lone_s"], got["t6"], got["ratio"], got["after_load"]))
    assert got["after_load"] == "8"
    assert got["arena_full"] == 0
    assert len(set(got["digests"])) == 1 and len(got["digests"]) == CONTEXTS, "the six passes computed different bytes"
    assert got["t6"] < 1.5 * got["t1"], "six passes took %.3f x a lone pass: they share hardware queues" % got["ratio"]


if __name__ == "__main__":
    child(int(sys.argv[1]) if len(sys.argv) > 1 else N)
