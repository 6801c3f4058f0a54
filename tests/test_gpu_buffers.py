"""The device buffers of one context on the GPU (csrc/eh_host.h, DevBuf): each grows after a smaller use and is reused unchanged
after a larger one, and every result equals the CPU oracle's.  The body is the one tests/test_emulated_buffers.py runs on the CPU
emulator (tests/hipemu/emu_buffers.py)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))

pytestmark = pytest.mark.gpu


def test_buffers_grow_and_are_reused():
    """n = 8, 200 without eh_reserve, 200 ordered twice (the arenas swap), 8 again, fuzz_calls 16 and 300 profiled, a corpus three
    times as large and the small one again: downloads, digests, first_of and selective downloads against the oracle"""
    import emu_buffers
    assert emu_buffers.run()
