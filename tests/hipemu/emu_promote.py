#!/usr/bin/env python3
"""Corpus promotion (erlamsa_amd/csrc/eh_promote.h: eh_corpus_promote, eh_corpus_promote_fresh, eh_corpus_download,
eh_selftest_promote) against a model that is Python alone: the corpus is a list of bytes objects, a promotion replaces it or adds to
it, the fresh selection is the header's rule written as a loop.  The second batches over a promoted corpus are held against the
oracle (tests/util.py oracle_batch) on the bytes the model says the corpus holds.

  ERLAMSA_HIP_LIB=build/liberlamsa_hip_emu.so python tests/hipemu/emu_promote.py

tests/test_emulated_promote.py runs it on the CPU wavefront emulator, tests/test_gpu_promote.py calls the same functions on the real
library.  With the emulator's race build (build_emu.py --race) as ERLAMSA_HIP_LIB the run also fails on any cross-lane access without
a rendezvous and on any access outside a device allocation."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
import numpy as np
import util
import emu_seen
import erlamsa_amd as ea
from erlamsa_amd import api, engine
from emu_unique import P, code, pack

# piece borders (P = 65 536) and vector-width borders
LENS = [0, 1, 15, 16, 17, 63, 64, 65, 1023, P - 1, P, P + 1, 2 * P + 5, 3 * P]
SMALL = [n for n in LENS if n < P - 1]
MUTATORS, PATTERNS = "sr,lr,num,bd", "od,nd"
OCAP = 8 << 20


# ---- the model --------------------------------------------------------------------------------------------------------------------
def fresh_rule(cases, status, cls, max_entry=0, max_total=0):
    """include/erlamsa_hip.h "Fresh": -> indices taken"""
    taken, s = [], 0
    for i, (b, st, c) in enumerate(zip(cases, status, cls)):
        if st != 0 or c != 0 or len(b) < 1 or (max_entry and len(b) > max_entry):
            continue
        s += len(b)
        if not max_total or s <= max_total:
            taken.append(i)
    return taken


def check_corpus(eng, entries, label=""):
    """eh_corpus_download (and the two size queries) against the model's entries, byte for byte"""
    data, off = eng.corpus_download()
    want = b"".join(entries)
    woff = np.zeros(len(entries) + 1, dtype=np.uint64)
    woff[1:] = np.cumsum([len(e) for e in entries], dtype=np.uint64)
    assert np.array_equal(off, woff), (label, off[:8], woff[:8])
    assert data.tobytes() == want, (label, util.first_diff(data.tobytes(), want))
    assert eng.corpus_size() == (len(entries), len(want)) and eng.corpus_device()[2:] == (len(entries), len(want)) and eng.n_corpus == len(entries), label


def arena(cases, lead=37):
    """the cases back to back behind `lead` bytes that belong to nobody: an arena that starts at an odd offset"""
    off = np.zeros(len(cases) + 1, dtype=np.uint64)
    off[0] = lead
    off[1:] = lead + np.cumsum([len(c) for c in cases], dtype=np.uint64)
    return np.frombuffer(b"\xa5" * lead + b"".join(cases) + b"\x5a", dtype=np.uint8), off


def planted_cases(n, rng):
    if n == 1:
        lens = [2 * P + 5]
    else:
        lens = (LENS + [SMALL[k % len(SMALL)] for k in range(n)])[:n]      # every length once, the piece-sized ones once only
    return [rng.integers(0, 256, size=k, dtype=np.uint8).tobytes() for k in lens]


# ---- 1. planted arenas ---------------------------------------------------------------------------------------------------------------
def planted_lists(n):
    """explicit lists over a planted arena of n cases: in order, reversed, with repeats, m = 0, both modes, append with room and
    append that must reallocate (a context of its own: its buffers are those of the 13-byte upload), a listed case that is not
    EH_CASE_OK, an index >= n.  -> promotions checked"""
    eng = ea.Engine(0)
    rng = np.random.Generator(np.random.PCG64(31 + n))
    cases = planted_cases(n, rng)
    status = np.zeros(n, dtype=np.int32)
    if n >= 64:
        status[[5, 20, 63]] = [1, 5, 2]
    ok = [i for i in range(n) if status[i] == 0]
    data, off = arena(cases)
    seed_corpus = [b"abc", b"0123456789"]                                  # 13 bytes: what is appended lands at an odd address
    done = 0

    def promote(corpus, idx, append, label):
        nonlocal done
        t, tb = eng.selftest_promote(data, off, status, idx=idx, append=append)
        corpus = (corpus if append else []) + [cases[i] for i in idx]
        assert (t, tb) == (len(idx), sum(len(cases[i]) for i in idx)), (label, t, tb)
        check_corpus(eng, corpus, (n, label))
        done += 1
        return corpus

    eng.upload_corpus(*pack(seed_corpus))
    addr = eng.corpus_device()[:2]
    corpus = promote(list(seed_corpus), ok, True, "append in order: must reallocate")
    assert sum(len(cases[i]) for i in ok) > 8192 and eng.corpus_device()[0] != addr[0]      # (13 bytes + 1.5x room: the upload's buffers cannot hold it)
    addr = eng.corpus_device()[:2]
    corpus = promote(corpus, ok[:3], True, "append into buffers with room")
    assert n == 1 or eng.corpus_device()[:2] == addr, "an append that fits must not allocate"
    corpus = promote(corpus, ok[::-1], False, "replace, reversed")
    rep = [ok[0], ok[-1], ok[0], ok[len(ok) // 2], ok[-1], ok[-1]]
    corpus = promote(corpus, rep, False, "replace, repeats")
    corpus = promote(corpus, [], True, "append, m = 0")
    corpus = promote(corpus, rep[::-1], True, "append, repeats")
    corpus = promote(corpus, [], False, "replace, m = 0")
    assert corpus == []
    corpus = promote(corpus, ok, False, "replace in order")
    # refused lists leave the corpus byte-identical
    assert code(eng.selftest_promote, data, off, status, idx=[0, n]) == -1
    if n >= 64:
        try:
            eng.selftest_promote(data, off, status, idx=[0, 20, 5])
            raise AssertionError("a listed case that is not EH_CASE_OK must be refused")
        except engine.EngineError as e:
            assert e.code == -1 and "case 20 " in str(e), e
    check_corpus(eng, corpus, (n, "after the refused lists"))
    eng.close()
    return done


def planted_fresh(eng, n):
    """the fresh selection over a planted arena of n cases with all four classes and other statuses mixed: no limits, max_entry_bytes
    equal to an entry's length and one less, max_total_bytes equal to S(k) and one less, a budget below the first eligible entry,
    nothing eligible; both modes.  -> promotions checked"""
    rng = np.random.Generator(np.random.PCG64(41 + n))
    cases = planted_cases(n, rng)
    status = np.zeros(n, dtype=np.int32)
    cls = np.zeros(n, dtype=np.uint8)
    if n >= 64:
        for i in range(n):
            cls[i] = (0, 0, 1, 0, 2, 0, 0, 3)[i % 8] if i >= len(LENS) else 0
        cls[[1, 3, 10]] = [1, 1, 2]                                         # (the first eligible entry has 15 bytes: a budget of 14 is a budget)
        status[cls == 3] = 5
        status[[4, 62]] = [2, 1]                                           # not EH_CASE_OK whatever their class says
    data, off = arena(cases, lead=5)
    elig = fresh_rule(cases, status, cls)
    assert elig and (n == 1 or len(elig) < n)
    sums = np.cumsum([len(cases[i]) for i in elig])
    k = len(elig) // 2
    limits = [(0, 0), (len(cases[elig[k]]), 0), (len(cases[elig[k]]) - 1, 0), (0, int(sums[k])), (0, int(sums[k]) - 1), (0, len(cases[elig[0]]) - 1),
              (len(cases[elig[-1]]), int(sums[k]))]
    corpus, done = [b"seed one", b"two"], 0
    eng.upload_corpus(*pack(corpus))
    for j, (me, mt) in enumerate(limits):
        append = j % 2 == 1
        want = fresh_rule(cases, status, cls, me, mt)
        t, tb = eng.selftest_promote(data, off, status, cls=cls, max_entry_bytes=me, max_total_bytes=mt, append=append)
        corpus = (corpus if append else []) + [cases[i] for i in want]
        assert (t, tb) == (len(want), sum(len(cases[i]) for i in want)), (n, me, mt, t, tb, len(want))
        check_corpus(eng, corpus, (n, "fresh", me, mt))
        done += 1
    assert fresh_rule(cases, status, cls, 0, len(cases[elig[0]]) - 1) == []          # (the budget below the first eligible entry took nothing)
    # nothing eligible: every class but 0, and class 0 with another status
    none = np.where(cls == 0, 1, cls).astype(np.uint8)
    for append in (True, False):
        assert eng.selftest_promote(data, off, status, cls=none, append=append) == (0, 0)
        corpus = corpus if append else []
        check_corpus(eng, corpus, (n, "nothing eligible", append))
    bad = np.full(n, 2, dtype=np.int32)
    assert eng.selftest_promote(data, off, bad, cls=np.zeros(n, dtype=np.uint8)) == (0, 0)
    return done + 3


def planted(eng):
    done = 0
    for n in (1, 64, 65, 130):
        done += planted_lists(n) + planted_fresh(eng, n)
    return done


# ---- 2. real batches -----------------------------------------------------------------------------------------------------------------
def seeds(n=64):
    return [("entry %d: value %d, ratio %d.%d\nsecond line of %d with 0x%x\n" % (i, i * 7919, i, i * 3, i, i * 31)).encode() for i in range(n)]


def against_oracle(eng, entries, label, **kw):
    """the engine's last batch against the oracle run over `entries` with the same options, under the skip rule of the parity tests"""
    data, off = pack(entries)
    ora = util.oracle_batch(data, off, max_case_bytes=OCAP, **kw)
    got, gst = eng.download()
    gdr, _ = eng.diag()
    assert len(got) == len(entries), label
    skip = [i for i in range(len(got)) if gst[i] in (2, 3) or ora.status[i] in (2, 3)]
    bad = [i for i in range(len(got)) if i not in skip and (gst[i] != ora.status[i] or not ora.same(i, got[i]) or (gst[i] == 0 and gdr[i] != ora.draws[i]))]
    assert not bad and len(skip) <= 1, (label, bad[:5], skip)
    return got, gst


def kept_of(outs, status):
    return [i for i, (o, s) in enumerate(zip(outs, status)) if s == 0 and len(o) > 0]


def real_explicit(n=64):
    """promote all EH_CASE_OK non-empty cases of a real batch, replace: the corpus is the concatenation of the downloaded outputs, the
    last batch's download is what it was, and a second batch over the promoted corpus is the oracle's over those bytes.  Then append:
    a batch whose corpus_first points into the appended part."""
    grew = 0
    for flags in (0, engine.EH_FLAG_ORDERED_OUTPUT):
        eng = ea.Engine(0)
        eng.configure(flags=flags, mutations=MUTATORS, patterns=PATTERNS)
        eng.upload_corpus(*pack(seeds(n)))
        eng.fuzz_batch(seed=(1, 2, 3), first_case=1)
        outs, status = against_oracle(eng, seeds(n), (flags, "batch 1"), seed=(1, 2, 3), first_case=1, mutations=MUTATORS, patterns=PATTERNS)
        idx = kept_of(outs, status)
        kept = [outs[i] for i in idx]
        grew += sum(1 for i in idx if len(outs[i]) > len(seeds(n)[i]))
        assert eng.corpus_promote(idx) == (len(kept), sum(map(len, kept)))
        check_corpus(eng, kept, (flags, "replace"))
        again, status2 = eng.download()
        assert again == outs and list(status2) == list(status), "the promotion changed the last batch's results"
        eng.fuzz_batch(seed=(1, 2, 3), first_case=n + 1)
        outs2, st2 = against_oracle(eng, kept, (flags, "batch 2 over the promoted corpus"), seed=(1, 2, 3), first_case=n + 1, mutations=MUTATORS, patterns=PATTERNS)
        # append: the corpus keeps its entries, the batch runs over the appended part alone
        idx2 = kept_of(outs2, st2)
        kept2 = [outs2[i] for i in idx2]
        eng.corpus_promote(idx2[::-1], append=True)
        check_corpus(eng, kept + kept2[::-1], (flags, "append"))
        assert eng.download()[0] == outs2
        eng.fuzz_batch(seed=(4, 5, 6), first_case=7, corpus_first=len(kept), n=len(kept2))
        against_oracle(eng, kept2[::-1], (flags, "batch 3 over the appended part"), seed=(4, 5, 6), first_case=7, mutations=MUTATORS, patterns=PATTERNS)
        eng.close()
    assert grew > 0, "no output of the workload grew: destinations were never further apart than the sources"


def real_fresh(n=64):
    """corpus_promote_fresh takes exactly what a host selection from result_seen's classes and the budget rule takes; a second call
    for the same batch promotes the same entries and records nothing twice; without a result_seen before it, it records the keys itself"""
    for flags in (0, engine.EH_FLAG_ORDERED_OUTPUT):
        eng = ea.Engine(0)
        eng.configure(flags=flags, mutations=MUTATORS, patterns=PATTERNS)
        eng.upload_corpus(*pack(seeds(n)))
        eng.seen_reserve(8 * n)
        model = emu_seen.Model(8 * n)
        eng.fuzz_batch(seed=(1, 2, 3), first_case=1)
        outs, status = eng.download()
        cls, _, _ = eng.result_seen(commit=True)
        wcls, _, _ = model.classify(outs, status)
        assert [int(c) for c in cls] == wcls
        lens = sorted(len(outs[i]) for i in fresh_rule(outs, status, cls))
        me = lens[(3 * len(lens)) // 4]
        mt = sum(lens[:len(lens) // 2])
        want = fresh_rule(outs, status, cls, me, mt)
        assert 0 < len(want) < len(fresh_rule(outs, status, cls, me, 0)) < len(lens), "the limits of the test limit nothing"
        held = eng.seen_count()
        for k in range(2):
            assert eng.corpus_promote_fresh(max_entry_bytes=me, max_total_bytes=mt) == (len(want), sum(len(outs[i]) for i in want)), (flags, k)
            check_corpus(eng, [outs[i] for i in want], (flags, "fresh", k))
            assert eng.seen_count() == held
        emu_seen.check_set(eng, model, "after two promotions")
        assert eng.download()[0] == outs
        # the next batch: the promotion classifies and records by itself, and result_seen afterwards returns the classes it used
        eng.fuzz_batch(seed=(1, 2, 3), first_case=n + 1)
        outs2, status2 = eng.download()
        wcls2, _, _ = model.classify(outs2, status2)
        want2 = fresh_rule(outs2, status2, wcls2)
        prev = [outs[i] for i in want]
        assert eng.corpus_promote_fresh(append=True) == (len(want2), sum(len(outs2[i]) for i in want2))
        check_corpus(eng, prev + [outs2[i] for i in want2], (flags, "fresh, append"))
        emu_seen.check_set(eng, model, "recorded by the promotion")
        cls2, _, _ = eng.result_seen(commit=True)
        assert [int(c) for c in cls2] == wcls2
        emu_seen.check_set(eng, model, "and once only")
        eng.close()


def real_attached(n=64):
    """a context that reads another's corpus (share_corpus): replace gives it an arena of its own, append copies the attached entries
    first; the owner's corpus is where and what it was"""
    owner = ea.Engine(0)
    owner.configure(mutations=MUTATORS, patterns=PATTERNS)
    owner.upload_corpus(*pack(seeds(n)))
    where = owner.corpus_device()
    for append in (False, True):
        eng = ea.Engine(0)
        eng.configure(mutations=MUTATORS, patterns=PATTERNS)
        eng.share_corpus(owner)
        assert eng.corpus_device() == where
        check_corpus(eng, seeds(n), "attached")
        eng.fuzz_batch(seed=(1, 2, 3), first_case=1)
        outs, status = eng.download()
        idx = kept_of(outs, status)
        eng.corpus_promote(idx, append=append)
        check_corpus(eng, (seeds(n) if append else []) + [outs[i] for i in idx], ("attached", append))
        assert eng.corpus_device()[0] != where[0]
        assert owner.corpus_device() == where
        check_corpus(owner, seeds(n), "the owner's corpus")
        eng.fuzz_batch(seed=(1, 2, 3), first_case=n + 1, corpus_first=n if append else 0, n=len(idx))
        against_oracle(eng, [outs[i] for i in idx], ("attached, next batch", append), seed=(1, 2, 3), first_case=n + 1, mutations=MUTATORS, patterns=PATTERNS)
        eng.close()
    owner.close()


def real_generators(n=16):
    """the file and jump generators point INTO the arena: a batch over a promoted corpus against the oracle with those bytes as Paths"""
    for gens in ("file", "jump"):
        eng = ea.Engine(0)
        eng.configure(mutations=MUTATORS, patterns=PATTERNS, generators=gens)
        eng.upload_corpus(*pack(seeds(n)))
        eng.fuzz_batch(seed=(3, 2, 1), first_case=1)
        outs, status = eng.download()
        idx = kept_of(outs, status)
        assert len(idx) >= 2
        eng.corpus_promote(idx)
        eng.fuzz_batch(seed=(3, 2, 1), first_case=n + 1)
        against_oracle(eng, [outs[i] for i in idx], gens, seed=(3, 2, 1), first_case=n + 1, mutations=MUTATORS, patterns=PATTERNS, generators=gens)
        eng.close()


def host_generations(inputs, opts, generations, keep, too_long=None):
    """the loop that needs no promotion: every generation is an api.fuzz_batch over what the host repacked from the one before"""
    cur, first, last = list(inputs), int(opts.get("first_case", 1)), None
    me = int(opts.get("max_entry_bytes", 0))
    for g in range(generations):
        last = api.fuzz_batch(cur, dict(opts, first_case=first), return_status=True)
        first += len(cur)
        if keep == "fresh":
            kept = [o for o, s, c in zip(*last) if s == 0 and c == 0 and len(o) > 0 and (not me or len(o) <= me)]
            if too_long is not None:
                too_long += [o for o, s, c in zip(*last) if s == 0 and c == 0 and me and len(o) > me]
        else:
            kept = [o for o, s in zip(last[0], last[1]) if s == 0 and len(o) > 0]
        if not kept:
            break
        cur = kept
    return last


def api_generations(n=16):
    """api.fuzz_generations(generations=3) for keep="all" and keep="fresh" equals the host loop of api.fuzz_batch calls"""
    opts = {"seed": (1, 2, 3), "mutations": MUTATORS, "patterns": PATTERNS}
    want = host_generations(seeds(n), opts, 3, "all")
    got = api.fuzz_generations(seeds(n), opts, generations=3, keep="all", return_status=True)
    assert got[0] == want[0] and list(got[1]) == list(want[1]) and len(got[0]) > 0
    assert api.fuzz_generations(seeds(n), opts, generations=3) == want[0]
    assert api.fuzz_generations(seeds(n), opts, generations=1, return_status=True)[0] == api.fuzz_batch(seeds(n), opts)
    fopts = dict(opts, fresh=4096, max_entry_bytes=80)
    api._engine(0).seen_reserve(0)
    too_long = []
    want = host_generations(seeds(n), fopts, 3, "fresh", too_long)
    api._engine(0).seen_reserve(0)
    got = api.fuzz_generations(seeds(n), fopts, generations=3, keep="fresh", return_status=True)
    assert got[0] == want[0] and list(got[1]) == list(want[1]) and list(got[2]) == list(want[2])
    assert 0 < len(got[0]) < n and too_long, "max_entry_bytes dropped nothing, or the set nothing"
    api._engine(0).seen_reserve(0)
    # the same refusals as fuzz_batch
    for bad in ({"sequence_muta": True}, {"external_post": object()}):
        try:
            api.fuzz_generations(seeds(2), dict(opts, **bad), generations=2)
            raise AssertionError("Unsupported expected")
        except api.Unsupported:
            pass
    # a campaign that promotes nothing stops: no fresh output of these seeds is one byte long
    one = dict(fopts, max_entry_bytes=1)
    want = host_generations(seeds(n), one, 3, "fresh")
    api._engine(0).seen_reserve(0)
    got = api.fuzz_generations(seeds(n), one, generations=3, keep="fresh", return_status=True)
    assert len(got[0]) == n and got[0] == want[0] and list(got[2]) == list(want[2]) and api._engine(0).corpus_size() == (0, 0)
    api._engine(0).seen_reserve(0)


def errors():
    """call order: EH_E_STATE before any batch, fresh without a reserved set, on a context that belongs to the coalescer, the download
    without a corpus; EH_E_INVALID for an index outside the batch, another mode, too small download buffers"""
    eng = ea.Engine(0)
    assert code(eng.corpus_download) == -5 and code(eng.corpus_size) == -5
    eng.configure(mutations="bd,bf", patterns="od")
    eng.upload_corpus(*pack([b"some input bytes"] * 8))
    assert code(eng.corpus_promote, [0]) == -5 and code(eng.corpus_promote_fresh) == -5           # no batch yet
    eng.fuzz_batch(seed=(1, 2, 3))
    assert code(eng.corpus_promote_fresh) == -5                                                   # no seen set
    assert code(eng.corpus_promote, [8]) == -1 and code(eng.corpus_promote, [0, 1 << 40]) == -1
    n, nb = ctypes.c_uint64(), ctypes.c_uint64()
    assert eng.lib.eh_corpus_promote(eng.h, None, 0, 2, ctypes.byref(n), ctypes.byref(nb)) == -1
    assert eng.lib.eh_corpus_promote_fresh(eng.h, 0, 0, 2, None, None) == -1
    buf, off = np.zeros(128, dtype=np.uint8), np.zeros(9, dtype=np.uint64)
    assert eng.lib.eh_corpus_download(eng.h, buf.ctypes.data, 127, off.ctypes.data, 9, None, None) == -1
    assert eng.lib.eh_corpus_download(eng.h, buf.ctypes.data, 128, off.ctypes.data, 8, None, None) == -1
    assert eng.lib.eh_corpus_download(eng.h, buf.ctypes.data, 128, off.ctypes.data, 9, ctypes.byref(n), ctypes.byref(nb)) == 0 and (n.value, nb.value) == (8, 128)
    check_corpus(eng, [b"some input bytes"] * 8, "nothing was promoted")
    eng.seen_reserve(64)
    t = eng.submit(b"a request", (1, 2, 3))
    arena1 = pack([b"abc"])
    for f, a, k in ((eng.corpus_promote, ([0],), {}), (eng.corpus_promote_fresh, (), {}), (eng.corpus_download, (), {}),
                    (eng.selftest_promote, (*arena1, np.zeros(1, dtype=np.int32)), {"idx": [0]})):
        assert code(f, *a, **k) == -5, f
    eng.flush()
    assert eng.poll(t) is not None
    eng.close()


def big_entry(eng):
    """(the device alone: minutes on the emulator) 256 planted entries, one of 8 MiB + 3 bytes = 129 pieces among small ones"""
    rng = np.random.Generator(np.random.PCG64(51))
    lens = [int(k) for k in rng.integers(0, 3000, size=256)]
    lens[100] = (8 << 20) + 3
    cases = [rng.integers(0, 256, size=k, dtype=np.uint8).tobytes() for k in lens]
    data, off = arena(cases, lead=3)
    eng.upload_corpus(*pack([b"odd"]))
    idx = list(range(255, -1, -1))
    assert eng.selftest_promote(data, off, np.zeros(256, dtype=np.int32), idx=idx, append=True) == (256, sum(lens))
    check_corpus(eng, [b"odd"] + cases[::-1], "a 129-piece entry")
    assert eng.selftest_promote(data, off, np.zeros(256, dtype=np.int32), cls=np.zeros(256, dtype=np.uint8)) == (sum(1 for k in lens if k), sum(lens))
    check_corpus(eng, [c for c in cases if c], "a 129-piece entry, fresh")


def race_report():
    return emu_seen.race_report()


def run():
    import time
    t0 = time.time()
    eng = ea.Engine(0)
    done = planted(eng)
    eng.close()
    for f in (real_explicit, real_fresh, real_attached, real_generators, api_generations, errors):
        print("%.0f s: %s" % (time.time() - t0, f.__name__), flush=True)
        f()
    return done


if __name__ == "__main__":
    done = run()
    rr = race_report()
    if rr is not None and rr != (0, 0):
        sys.exit("race build: %d cross-lane accesses without a rendezvous, %d accesses outside a device allocation" % rr)
    print("promote ok: %d planted promotions%s" % (done, "" if rr is None else ", race build clean"))
