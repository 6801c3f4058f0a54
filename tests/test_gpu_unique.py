"""The uniqueness filter on the GPU (csrc/eh_unique.h; include/erlamsa_hip.h eh_result_digests, eh_result_unique,
eh_result_download_select, eh_selftest_unique).  Expected values come from Python alone - zlib.crc32, a table CRC-32C pinned by its
check value, a dict keyed by bytes - and the bodies are those tests/test_emulated_unique.py runs on the CPU emulator."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def uq():
    import emu_unique
    emu_unique.piece_size_is_the_headers()
    return emu_unique


@pytest.fixture(scope="module")
def eng(uq):
    e = uq.ea.Engine(0)
    yield e
    e.close()


def test_digests_of_planted_lengths(uq, eng):
    """0 .. 1025 bytes, around one and two pieces, more pieces than lanes, all-zero and all-0xFF, at odd arena offsets"""
    assert uq.digests_of_planted_lengths(eng) == 19


def test_dedup_of_planted_cases(uq, eng):
    """duplicates near and far, near misses, empties, other statuses, multi-piece cases, a constructed digest collision"""
    assert uq.dedup_of_planted_cases(eng) >= 90


def test_real_batches_digests_unique_and_selective_download(uq):
    """4096 cases, seed (1, 2, 3): an HTTP request under the default tables and a random block under the byte mutators, with and
    without EH_FLAG_ORDERED_OUTPUT; at least 5 % of the EH_CASE_OK cases are duplicates; a second batch invalidates the cache"""
    shares = uq.end_to_end(4096)
    assert len(shares) == 4


def test_unique_option_of_the_api(uq):
    uq.api_option(4096)


def test_call_order_and_argument_errors(uq):
    uq.errors()
