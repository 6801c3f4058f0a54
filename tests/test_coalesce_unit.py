"""The request coalescer's bookkeeping (csrc/eh_coalesce.h: the pending batch, where a ticket is, launched / collected / cancel)
without the engine: a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer that holds it against a naive
model (tests/hipemu/coalesce_unit.cpp)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))


def test_coalescer_bookkeeping_against_a_model():
    """erase at every position of a batch of 0, 5, 0 and 300 bytes, 2 000 random pushes and erases, the two flush limits at and
    one below, where() in all four states, launched, collected with two of six tickets cancelled, cancel in every state: no
    failed check and no sanitizer report"""
    import build_emu
    exe = build_emu.build_coalesce_unit()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.splitlines()[-1] == "coalesce_unit ok", r.stdout[-2000:]
