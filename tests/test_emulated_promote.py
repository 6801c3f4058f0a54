"""Corpus promotion (csrc/eh_promote.h: outputs of the last batch become corpus entries on the device) on the CPU wavefront emulator:
the kernels unmodified, expected values from a Python model alone and, for the batches over a promoted corpus, from the oracle
(tests/hipemu/emu_promote.py).  tests/test_gpu_promote.py runs the same bodies on the gfx950 binary."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))


def test_emulated_corpus_promotion():
    """planted arenas of 1, 64, 65 and 130 cases through eh_selftest_promote (piece and vector-width borders, odd source and
    destination addresses, explicit lists and the fresh selection under both limits, both modes, append with and without room), two
    real batches of 64 cases with and without EH_FLAG_ORDERED_OUTPUT against the oracle, an attached corpus, the file and jump
    generators over a promoted corpus, api.fuzz_generations against the host loop, call order errors"""
    import build_emu
    env = dict(os.environ, ERLAMSA_HIP_LIB=build_emu.build())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hipemu", "emu_promote.py")], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "promote ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
