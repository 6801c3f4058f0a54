#!/usr/bin/env python3
"""The device buffers of ONE context through a life in which every one of them grows after a smaller use and is reused unchanged
after a larger one (erlamsa_amd/csrc/eh_host.h, DevBuf): result arrays, slots, both arenas, ordered offsets, bounce buffers,
seeds and profile ids, the uniqueness filter's arrays, the selection list, the corpus.  Every result is held against the CPU oracle.

  ERLAMSA_HIP_LIB=build/liberlamsa_hip_emu.so python tests/hipemu/emu_buffers.py

tests/test_emulated_buffers.py runs it on the CPU wavefront emulator, tests/test_gpu_buffers.py calls run() on the real library."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
import numpy as np
import pyoracle as po
import erlamsa_amd as ea
from erlamsa_amd import engine
from emu_unique import digests_of, first_occurrences

MUTATORS, PATTERNS = "bd,bf,bi,sr,ld", "od,nd"
# `sr` repeats a stretch of its block up to 2^10 times and `nd` lets it do so again and again: one case in twenty of a batch of
# random blocks grows past any slot.  This test is about the host's buffers, not about the work areas, so its seeds are the ones
# under which the ORACLE ALONE keeps every case within CALM bytes (batch seeds: found by running it over the corpora below; per-case
# seeds: calm_seeds() draws again for the cases that grow).  Slots are four times that, the oracle's guard is set to the slot, and
# oracle() asserts that no case met it - so every case is compared, status and bytes, and none is left out.
CALM, MCB = 256 << 10, 1 << 20
SEED_A, SEED_B = (10, 11, 12), (28, 29, 30)
CONF = dict(mutations=MUTATORS, patterns=PATTERNS, max_case_bytes=MCB, pool_bytes=256 << 20)
# profile 0 is the configuration; two more are added between the two fuzz_calls
PROFILES = [(MUTATORS, PATTERNS, 1.0), ("bd,bi", "od", 1.0), ("sr,ld,bf", "nd", 0.5)]


def corpus(n, size, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [rng.integers(0, 256, size=size, dtype=np.uint8).tobytes() for _ in range(n)]


def oracle(inputs, seed=None, seeds=None, ids=None):
    """-> (outs, status, draws) in case order; with ids, one oracle run per profile over that profile's own cases"""
    n = len(inputs)
    ids = [0] * n if ids is None else [int(x) for x in ids]
    outs, st, dr = [None] * n, [0] * n, [0] * n
    for k in sorted(set(ids)):
        idx = [i for i in range(n) if ids[i] == k]
        d, o = po.pack([inputs[i] for i in idx])
        m, p, b = PROFILES[k]
        kw = {"seed": seed} if seeds is None else {"seeds": np.asarray(seeds)[idx]}
        r = po.fuzz_batch(d, o, mutations=m, patterns=p, blockscale=b, max_case_bytes=MCB, **kw)
        for j, i in enumerate(idx):
            outs[i], st[i], dr[i] = r[0][j], int(r[1][j]), int(r[2][j])
    assert all(s in (0, 1) for s in st) and max(map(len, outs)) <= CALM, "pick other seeds: a case grows past CALM in the oracle itself"
    return outs, st, dr


def calm_seeds(inputs, ids, rng):
    """per-case seeds under which no case grows past CALM bytes in the oracle: drawn again for the cases that do"""
    n = len(inputs)
    seeds = rng.integers(1, 100000, size=(n, 3)).astype(np.int64)
    for _ in range(16):
        loud = []
        for k in sorted(set(int(x) for x in ids)):
            idx = [i for i in range(n) if int(ids[i]) == k]
            d, o = po.pack([inputs[i] for i in idx])
            m, p, b = PROFILES[k]
            outs, st, _, _ = po.fuzz_batch(d, o, seeds=seeds[idx], mutations=m, patterns=p, blockscale=b, max_case_bytes=MCB)
            loud += [i for j, i in enumerate(idx) if int(st[j]) not in (0, 1) or len(outs[j]) > CALM]
        if not loud:
            return seeds
        seeds[loud] = rng.integers(1, 100000, size=(len(loud), 3))
    raise AssertionError("no calm seeds after 16 rounds")


def check(eng, label, want, select=None):
    """the last batch of `eng` against the oracle's (outs, status, draws): download, diag, digests, unique, and download_select of
    the listed cases"""
    outs, st, dr = want
    got, gst = eng.download()
    assert [int(s) for s in gst] == st, (label, "status")
    bad = [i for i in range(len(outs)) if got[i] != outs[i]]
    assert not bad, (label, "bytes differ", bad[:10])
    draws, _ = eng.diag()
    assert [int(d) for d, s in zip(draws, st) if s == 0] == [d for d, s in zip(dr, st) if s == 0], (label, "draws")
    assert [int(d) for d in eng.digests()] == digests_of(outs), (label, "digests")
    first, n_unique, unique_bytes = eng.unique()
    wfirst = first_occurrences(outs, st)
    uniq = [i for i in range(len(outs)) if st[i] == 0 and wfirst[i] == i]
    assert [int(f) for f in first] == wfirst, (label, "first_of")
    assert (n_unique, unique_bytes) == (len(uniq), sum(len(outs[i]) for i in uniq)), (label, "unique totals")
    if select is not None:
        assert eng.download_select(select) == [outs[i] for i in select], (label, "download_select")
    print("%s: %d cases, %d output bytes, %d distinct" % (label, len(outs), sum(map(len, outs)), len(uniq)))


def run():
    small, large, wide = corpus(8, 64, 31), corpus(200, 256, 32), corpus(200, 768, 33)
    # the 300 calls are 150 (input, seed, profile) triples, each made twice: half the batch repeats the other half
    calls16, calls300 = corpus(16, 64, 34), corpus(150, 64, 35) * 2
    rng = np.random.Generator(np.random.PCG64(36))
    ids300 = np.arange(300, dtype=np.uint32) % 150 % 3
    seeds16 = calm_seeds(calls16, [0] * 16, rng)
    seeds300 = np.concatenate([calm_seeds(calls300[:150], ids300[:150], rng)] * 2)
    want_small, want_large, want_large2 = oracle(small, SEED_A), oracle(large, SEED_A), oracle(large, SEED_B)

    eng = ea.Engine(0)
    eng.configure(**CONF)
    # 1. the first, small use of everything
    eng.upload_corpus(*po.pack(small))
    eng.fuzz_batch(seed=SEED_A)
    check(eng, "n = 8", want_small, select=[7, 0])
    # 2. every per-case buffer, the slots, the arena (8 x input bytes + 2 GiB) and the corpus grow: no eh_reserve
    eng.upload_corpus(*po.pack(large))
    eng.fuzz_batch(seed=SEED_A)
    assert eng.download_select([199, 0, 77]) == [want_large[0][i] for i in (199, 0, 77)]
    check(eng, "n = 200", want_large)
    # 3. case-ordered output: the second arena and the ordered offsets appear, the arenas swap roles after every batch, and
    #    the bounce buffers are made again for chunks of 512 bytes
    eng.configure(flags=engine.EH_FLAG_ORDERED_OUTPUT, download_chunk_bytes=512, **CONF)
    eng.fuzz_batch(seed=SEED_A)
    check(eng, "n = 200, ordered", want_large, select=[199, 0, 77])
    eng.fuzz_batch(seed=SEED_B)
    check(eng, "n = 200, ordered, arenas swapped", want_large2, select=list(range(0, 200, 7)))
    # 4. the small batch again, in buffers that are all larger than it needs
    eng.upload_corpus(*po.pack(small))
    eng.fuzz_batch(seed=SEED_A)
    check(eng, "n = 8 again", want_small, select=[7, 0])
    # 5. per-case seeds: the seed buffer's first use, then a larger one with profile ids behind the seeds
    eng.upload_corpus(*po.pack(calls16))
    eng.fuzz_calls(seeds16)
    check(eng, "fuzz_calls n = 16", oracle(calls16, seeds=seeds16))
    assert [eng.profile_add(*p) for p in PROFILES] == [0, 1, 2]
    eng.upload_corpus(*po.pack(calls300))
    eng.fuzz_calls(seeds300, ids300)
    check(eng, "fuzz_calls n = 300, profiled", oracle(calls300, seeds=seeds300, ids=ids300), select=[299, 150, 1])
    # 6. a corpus three times as large as any before (new buffers), then the small one (the buffers stay)
    eng.upload_corpus(*po.pack(wide))
    eng.fuzz_batch(seed=SEED_A)
    check(eng, "n = 200 of 768 bytes", oracle(wide, SEED_A))
    eng.upload_corpus(*po.pack(small))
    eng.fuzz_batch(seed=SEED_A)
    check(eng, "n = 8 at the end", want_small, select=[7, 0])
    eng.close()
    return True


if __name__ == "__main__":
    run()
    print("buffers ok")
