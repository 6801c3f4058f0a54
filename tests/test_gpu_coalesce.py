"""Request coalescing from several threads on the GPU (csrc/eh_coalesce.h and the coalescer of csrc/eh_host_coalesce.h): submitters, pollers
and a flusher share one context, and every ticket gets the bytes its request gets alone, which are the CPU oracle's.  The body is
the one tests/test_emulated_kernel.py runs on the CPU emulator (tests/hipemu/emu_coalesce_threads.py)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))

pytestmark = pytest.mark.gpu


def test_coalescing_from_threads():
    """4 client threads of 24 requests of at most 300 bytes, a flusher thread, a launch every 16 requests: a collector downloads
    with the lock released while the others keep submitting and polling; statuses and bytes against the oracle"""
    import emu_coalesce_threads
    assert emu_coalesce_threads.run()
