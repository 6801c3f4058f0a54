"""The seen set on the GPU (csrc/eh_seen.h; include/erlamsa_hip.h eh_seen_reserve, eh_seen_count, eh_seen_add_keys,
eh_seen_add_corpus, eh_seen_export, eh_result_seen, eh_selftest_seen).  Expected values come from a Python model alone - a set of
(len(bytes), digest) carried across batches, zlib.crc32 and a table CRC-32C - and the bodies are those
tests/test_emulated_seen.py runs on the CPU emulator."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sn():
    import emu_seen
    return emu_seen


@pytest.fixture(scope="module")
def eng(sn):
    e = sn.ea.Engine(0)
    yield e
    e.close()


def test_planted_batches_across_the_rank_steps(sn, eng):
    """65, 130 and 1 cases against a capacity-64 set: classes, counters and the export order equal the model's"""
    assert sn.planted_batches(eng) == 196


def test_tiny_tables_and_a_full_set(sn, eng):
    """8 and 2 slots: wrapping probe chains, the first keys by case index are kept, the rest counted, nothing unseen called seen"""
    sn.tiny_tables(eng)


def test_commit_and_idempotence_per_batch(sn, eng):
    sn.idempotence_and_commit(eng)


def test_keys_from_outside_and_from_the_corpus(sn, eng):
    sn.keys_from_outside(eng)


def test_two_real_batches_against_the_model(sn):
    """1024 cases twice (cases 1..1024 and 1025..2048 of one run, seed (1, 2, 3)), the set seeded with the corpus, with and without
    EH_FLAG_ORDERED_OUTPUT.  The oracle's counts for the second batch: 662 fresh, 271 repeats inside the batch, 91 seen before, 0 not
    EH_CASE_OK (8.9 % and 64.6 % of the EH_CASE_OK cases in classes 2 and 0; the test wants 5 % of each)."""
    shares = sn.real_batches(1024)
    assert len(shares) == 2


def test_fresh_option_of_the_api(sn):
    sn.api_option(1024)


def test_call_order_errors_and_small_export_buffer(sn):
    sn.errors()
