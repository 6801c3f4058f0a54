"""Option profiles (eh_profile_add, eh_fuzz_calls_profiled, eh_submit_profiled: mutations / patterns / blockscale per case of one
launch) on the CPU wavefront emulator: the kernel unmodified, expected bytes from the oracle run once per profile
(tests/hipemu/emu_profiles.py).  tests/test_gpu_profiles.py runs the same bodies on the gfx950 binary."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))


def test_emulated_option_profiles():
    """64 interleaved cases against the oracle and against every profile alone, the shapes where the table indexing can go wrong,
    64 coalesced requests from four threads with a profile added while a batch is in flight, interning / limits / errors,
    api.fuzz_requests against api.fuzz one by one"""
    import build_emu
    env = dict(os.environ, ERLAMSA_HIP_LIB=build_emu.build())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hipemu", "emu_profiles.py"), "64"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "profiles ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
