"""The uniqueness filter (csrc/eh_unique.h: digests, duplicates, selective download) on the CPU wavefront emulator: the kernels
unmodified, expected values from Python alone (tests/hipemu/emu_unique.py).  tests/test_gpu_unique.py runs the same bodies on the
gfx950 binary."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))


def test_emulated_uniqueness_filter():
    """planted lengths and duplicates through eh_selftest_unique, two real batches of 64 cases with and without
    EH_FLAG_ORDERED_OUTPUT, the `unique` option of the API, call order and argument errors"""
    import build_emu
    env = dict(os.environ, ERLAMSA_HIP_LIB=build_emu.build())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hipemu", "emu_unique.py"), "64"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "unique ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
