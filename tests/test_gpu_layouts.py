"""The memory that the kernels and the host ABI address by position (csrc/eh_common.h: BatchCounters, BatchSummary, PoolCounters,
CoBoard::stat), read back through the ABI after one batch and checked against the per-case arrays of the same batch.  A member
that moved on one side only shows here as a total that is not the sum of its cases."""
import ctypes as C

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

# (slots of 2 MiB and a pool of its own size, so that no other context of the process shares the pool: tiers of 4, 8, 16, 32 and
# 64 MiB - twice the area per tier up to big_case_bytes, whose default is 32 slots' worth)
MCB, POOL, TIERS = 2 << 20, 192 << 20, 5
SEED = (1, 2, 3)


def test_totals_are_the_sums_of_the_cases():
    """64 cases of 256 random bytes, default tables: summary, occupancy, pool and board statistics against lengths and statuses;
    then a batch of no cases, whose summary the host stamps itself"""
    import erlamsa_amd as ea
    data = np.frombuffer(b"".join(util.corpus_uniform(64, 256)), dtype=np.uint8)
    off = np.arange(65, dtype=np.uint64) * 256
    eng = ea.Engine(0)
    try:
        eng.configure(max_case_bytes=MCB, pool_bytes=POOL)
        eng.upload_corpus(data, off)
        eng.fuzz_batch(seed=SEED)
        outs, status = eng.download()
        lengths = np.array([len(o) for o in outs], dtype=np.int64)
        in_bytes, out_bytes, cases, by_status = eng.summary()
        print("summary", in_bytes, out_bytes, cases, by_status.tolist(), "lengths", int(lengths.sum()), "statuses", np.bincount(status, minlength=6).tolist())
        assert in_bytes == 64 * 256
        assert out_bytes == int(lengths.sum())
        assert cases == 64
        assert by_status.tolist() == np.bincount(status, minlength=6).tolist()

        held, in_cases, lingering, workgroups, wave_slots = eng.occupancy()
        print("occupancy", held, in_cases, lingering, workgroups, wave_slots)
        assert 0 < in_cases <= held
        assert 1 <= workgroups <= 64

        raw = np.zeros(64, dtype=np.uint64)
        assert eng.lib.eh_pool_stats(eng.h, raw.ctypes.data_as(C.c_void_p)) == 0
        ps = eng.pool_stats()
        print("pool", ps)
        assert int(raw[40]) == TIERS and ps["area_bytes"] == [MCB << t for t in range(1, TIERS + 1)]
        assert ps["contexts"] == 1

        co = np.full(8, 0xDEADBEEF, dtype=np.uint64)
        assert eng.lib.eh_coop_stats(eng.h, co.ctypes.data_as(C.c_void_p)) == 0
        print("coop", co.tolist())
        assert len(co) == 8 and int(co[4]) == 0 and not (co[5:] != 0).any()      # no loop found the board full; words 5 .. 7 are unused
        assert eng.coop_stats()["board_full"] == 0

        eng.fuzz_batch(seed=SEED, n=0)                                           # no mutate kernel runs: `seq` comes from the host
        in_bytes, out_bytes, cases, by_status = eng.summary()
        assert (in_bytes, out_bytes, cases, by_status.tolist()) == (0, 0, 0, [0] * 6)
    finally:
        eng.close()
