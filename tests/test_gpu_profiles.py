"""Option profiles on the GPU (include/erlamsa_hip.h eh_profile_add, eh_profile_count, eh_fuzz_calls_profiled, eh_submit_profiled):
cases of one launch under different mutations / patterns / blockscale.  Expected bytes come from the CPU oracle, one run per profile
over that profile's own cases; the bodies are those tests/test_emulated_profiles.py runs on the CPU emulator."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))

pytestmark = pytest.mark.gpu

N, REQUESTS = 256, 300


@pytest.fixture(scope="module")
def pf():
    import emu_profiles
    return emu_profiles


def test_interleaved_profiles_match_the_oracle(pf):
    """256 cases, case i under profile i % 4, per-case seeds with (0,0,0) and a negative triple: status, bytes and draws"""
    assert pf.parity(N) >= 0.97 * N


def test_profiled_batch_equals_each_profile_alone(pf):
    """engine against engine, nothing left out: statuses, bytes, draws, last mutators; all ids 3; all ids 0 against plain fuzz_calls"""
    assert pf.alone(N) == N


def test_shapes_where_the_table_indexing_can_go_wrong(pf):
    """n = 1, n = 65 with the id changing at case 64, one mutator / one pattern, every GPU mutator under a work budget"""
    assert pf.shapes(N)


def test_flags_and_uniqueness_filter_over_a_profiled_batch(pf):
    """EH_FLAG_ORDERED_OUTPUT, EH_FLAG_META_TRACE (the trace text of one case per profile), Engine.unique()"""
    assert pf.shapes_flags(N)


def test_coalesced_requests_of_different_profiles(pf):
    """300 requests from four threads, a fifth profile added while a batch is in flight, two cancelled tickets, random poll order"""
    assert pf.coalescer(REQUESTS) == REQUESTS - 2


def test_interning_limits_and_errors(pf):
    assert pf.interning_limits_errors()


def test_fuzz_requests_of_the_api(pf):
    """32 requests with mixed options in one launch = api.fuzz one by one on a fresh engine"""
    assert pf.api_requests()
