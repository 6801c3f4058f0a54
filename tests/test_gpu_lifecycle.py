"""The life of a context on the GPU (csrc/eh_host.h: the parts of a context own their events, streams and page-locked memory):
contexts that make every lazily created handle and buffer are destroyed one after the other, and each computes what the first
one and the CPU oracle computed.  tests/hipemu/host_lifecycle.cpp walks the same calls under AddressSanitizer on the CPU
emulator, whose streams are null handles: stream and event ownership is exercised here."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

MUTATORS, PATTERNS = "bd,bf,bi,sr", "od,nd"
# (slots of 1 MiB and a small pool: three contexts are made and destroyed.  Under SEED and SEEDS the oracle keeps every case far
# below the slot, so every case is compared and none ends with an engine-only status; the test asserts it.)
MCB = 1 << 20
CONF = dict(mutations=MUTATORS, patterns=PATTERNS, max_case_bytes=MCB, pool_bytes=256 << 20)
SEED = (1, 2, 3)
SEEDS = np.array([[5, 6, 7 + k] for k in range(4)], dtype=np.int64)
SELECT = [7, 0, 3]


def _round(ea, engine, inputs, data, off):
    """create .. destroy -> everything the round read back"""
    eng = ea.Engine(0)
    eng.configure(flags=engine.EH_FLAG_META_TRACE, **CONF)
    eng.upload_corpus(data, off)
    eng.reserve(len(inputs))
    eng.fuzz_batch(seed=SEED)
    outs, status = eng.download()                            # the gather and copy streams, their events, the bounce buffers
    select = eng.download_select(SELECT)
    summary = eng.summary()                                  # the page-locked totals
    first_of, n_unique, unique_bytes = eng.unique()
    eng.seen_reserve(64)
    cls, n_fresh, fresh_bytes = eng.result_seen(commit=True)
    stream = eng.own_stream()                                # the context's own stream
    tickets = [eng.submit(inputs[k], tuple(int(x) for x in SEEDS[k])) for k in range(4)]
    eng.flush()
    polled = [eng.poll(t, cap=MCB) for t in tickets]
    eng.configure(flags=engine.EH_FLAG_ORDERED_OUTPUT, **CONF)   # the second arena and the ordered offsets
    eng.upload_corpus(data, off)                             # (the coalescer's batch replaced the corpus)
    eng.fuzz_batch(seed=SEED, stream=stream)
    outs2, status2 = eng.download()
    eng.close()
    return dict(outs=list(outs), status=[int(s) for s in status], select=select, summary=(summary[:3], [int(x) for x in summary[3]]),
                first_of=[int(f) for f in first_of], unique=(n_unique, unique_bytes), cls=[int(c) for c in cls], fresh=(n_fresh, fresh_bytes),
                polled=polled, outs2=list(outs2), status2=[int(s) for s in status2])


def test_contexts_come_and_go():
    """three rounds of create -> batch, download, selective download, summary, filter, seen set, own stream, coalesced requests,
    ordered batch on the own stream -> destroy, on 64 inputs of 256 bytes: every round's bytes and statuses are the first
    round's and the oracle's, and no call returns an error (the binding raises on one)"""
    import pyoracle as po
    inputs = util.corpus_uniform(64, 256)
    data, off = po.pack(inputs)
    okw = dict(mutations=MUTATORS, patterns=PATTERNS, max_case_bytes=MCB)
    ora = util.oracle_batch(data, off, seed=SEED, **okw)
    d4, o4 = po.pack(inputs[:4])
    ora4 = util.oracle_batch(d4, o4, seeds=SEEDS, **okw)
    for o in (ora, ora4):
        assert all(int(s) in (0, 1) for s in o.status) and int(max(o.lens)) <= MCB // 4, "pick other seeds: a case grows towards the slot in the oracle itself"
    if util.priming():
        pytest.skip("oracle cache primed")
    import erlamsa_amd as ea
    from erlamsa_amd import engine
    first = None
    for r in range(3):
        got = _round(ea, engine, inputs, data, off)
        if first is None:
            first = got
            want = [int(s) for s in ora.status]
            for outs, status in ((got["outs"], got["status"]), (got["outs2"], got["status2"])):
                assert status == want, "statuses differ from the oracle's"
                bad = [i for i in range(len(inputs)) if not ora.same(i, outs[i])]
                assert not bad, ("bytes differ from the oracle's", bad[:10])
            assert all(ora.same(i, b) for i, b in zip(SELECT, got["select"])), "download_select differs from the oracle's"
            assert [p[0] for p in got["polled"]] == [int(s) for s in ora4.status], "coalesced requests: statuses differ from the oracle's"
            assert all(ora4.same(k, got["polled"][k][1]) for k in range(4)), "coalesced requests: bytes differ from the oracle's"
            assert got["summary"][0] == (256 * 64, int(sum(ora.lens)), 64)
        else:
            diff = [k for k in first if got[k] != first[k]]
            assert not diff, "round %d differs from the first in %s" % (r + 1, diff)
