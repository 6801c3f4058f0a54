"""The seen set (csrc/eh_seen.h: keys of earlier batches' outputs kept on the device) on the CPU wavefront emulator: the kernels
unmodified, expected values from a Python model alone (tests/hipemu/emu_seen.py).  tests/test_gpu_seen.py runs the same bodies on
the gfx950 binary."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))


def test_emulated_seen_set():
    """planted batches of 65, 130 and 1 cases through eh_selftest_seen, tables of 8 and 2 slots, commit and idempotence, keys from
    outside and from the corpus, two consecutive real batches of 64 cases with and without EH_FLAG_ORDERED_OUTPUT, the `fresh`
    option of the API, call order errors"""
    import build_emu
    env = dict(os.environ, ERLAMSA_HIP_LIB=build_emu.build())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hipemu", "emu_seen.py"), "64"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "seen ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
