"""Corpus promotion on the GPU (csrc/eh_promote.h; include/erlamsa_hip.h eh_corpus_promote, eh_corpus_promote_fresh,
eh_corpus_download, eh_selftest_promote).  Expected values come from a Python model alone - the corpus as a list of bytes objects, the
fresh rule as a loop - and from the oracle for the batches that run over a promoted corpus; the bodies are those
tests/test_emulated_promote.py runs on the CPU emulator."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pm():
    import emu_promote
    return emu_promote


@pytest.fixture(scope="module")
def eng(pm):
    e = pm.ea.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_planted_lists_across_the_scan_steps(pm, n):
    """in order, reversed, repeats, m = 0, both modes, append with room and append that reallocates, refused lists"""
    assert pm.planted_lists(n) == 8


@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_planted_fresh_selection_under_both_limits(pm, eng, n):
    assert pm.planted_fresh(eng, n) == 10


def test_an_entry_of_129_pieces_among_small_ones(pm, eng):
    """256 planted entries, one of 8 MiB + 3 bytes, promoted in reversed order behind a 3-byte corpus and by the fresh selection"""
    pm.big_entry(eng)


def test_explicit_promotion_of_real_batches_against_the_oracle(pm):
    pm.real_explicit()


def test_fresh_promotion_of_real_batches_against_the_seen_model(pm):
    pm.real_fresh()


def test_promotion_on_an_attached_corpus_leaves_the_owner_alone(pm):
    pm.real_attached()


def test_file_and_jump_generators_over_a_promoted_corpus(pm):
    pm.real_generators()


def test_fuzz_generations_equals_the_host_loop(pm):
    pm.api_generations()


def test_call_order_errors(pm):
    pm.errors()
