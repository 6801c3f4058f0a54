#!/usr/bin/env python3
"""Option profiles (include/erlamsa_hip.h eh_profile_add, eh_fuzz_calls_profiled, eh_submit_profiled): cases of ONE launch that run
under different mutations / patterns / blockscale, as the requests of erlamsa's HTTP service do (erlamsa_esi.erl:30-68).  Expected
bytes come from the CPU oracle, one run per profile over that profile's own cases; the engine is also held against itself (a
profiled batch = every profile alone on a context configured with it).

  ERLAMSA_HIP_LIB=build/liberlamsa_hip_emu.so python tests/hipemu/emu_profiles.py [cases]

tests/test_emulated_profiles.py runs it on the CPU wavefront emulator (64 cases), tests/test_gpu_profiles.py calls the same
functions on the real library (256 cases, 300 coalesced requests)."""
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import pyoracle as po
import util
import erlamsa_amd as ea
from erlamsa_amd import api, engine
from erlamsa_amd.engine import EngineError

MCB = 8 << 20                                      # max_case_bytes of every context and oracle run here
# (mutations, patterns, blockscale); the first is what the contexts are configured with = profile 0
PROFILES = [("bd,bf,bi,sr,sd,num,ld,lr,ab,uw", "od,nd,bu", 1.0),
            ("num=5,ld,lr2,lis", "od", 0.5),
            ("sr,sd,sp,snand,srnd,tr2,td", "nd,bu,sk", 2.0),
            ("uw,ui,ab,ad,len", "bu,nu,co", 0.1)]
FIFTH = ("bd,bf=3,sr", "od,nd", 1.5)               # added while a coalesced batch is in flight
# Corpus and seed constants: util.corpus_mixed(n, 400, seed=25) with the seeds below gives NO status 2 or 3 in the oracle under any
# of the four profiles, at n = 64 and at n = 256 (found by running the oracle alone); the 3 % cap of parity() therefore guards
# engine-side limits only.
CORPUS_SEED, SEEDS_SEED = 25, 9
LEFT_OUT_CAP = 0.03                                # the cap of tests/test_gpu_parity.py test_per_call_seeds_mode


def code(f, *a, **k):
    try:
        f(*a, **k)
    except EngineError as e:
        return e.code
    return 0


def seeds_of(n):
    """per-case seeds as test_per_call_seeds_mode makes them: (0,0,0), the AS183 moduli and a negative triple among them"""
    rng = np.random.Generator(np.random.PCG64(SEEDS_SEED))
    seeds = rng.integers(0, 99999, size=(n, 3)).astype(np.int64) + 1
    for k, s in enumerate([(0, 0, 0), (30268, 30306, 30322), (-5, 7, -9)][:n]):
        seeds[k] = s
    return seeds


def oracle(inputs, seeds, ids, profiles, trace=False, **kw):
    """one oracle run per profile over that profile's own cases -> (outs, status, draws, trace per case), in case order"""
    n = len(inputs)
    outs, st, dr, tr = [None] * n, np.zeros(n, np.int32), np.zeros(n, np.uint64), [None] * n
    for k in sorted(set(int(x) for x in ids)):
        idx = [i for i in range(n) if int(ids[i]) == k]
        d, o = po.pack([inputs[i] for i in idx])
        m, p, b = profiles[k]
        r = po.fuzz_batch(d, o, seeds=np.asarray(seeds)[idx], mutations=m, patterns=p, blockscale=b, max_case_bytes=MCB, trace=trace, **kw)
        lines = r[3].split("\x1e\n") if trace == "full" else [None] * len(idx)
        for j, i in enumerate(idx):
            outs[i], st[i], dr[i], tr[i] = r[0][j], r[1][j], r[2][j], lines[j]
    return outs, st, dr, tr


_workloads, _mixed, _keep = {}, {}, []


def keep_pool():
    """One context stays open for the whole run: the device's work-area pool (a quarter of its memory) lives as long as a context of
    its sizes does, and every context here has them - without this each of the dozen contexts below would make and free it again."""
    if not _keep:
        eng = ea.Engine(0)
        eng.configure(mutations="bd", patterns="od", max_case_bytes=MCB)
        data, off = po.pack([b"keep"])
        eng.upload_corpus(data, off)
        eng.fuzz_batch(seed=(1, 2, 3))
        eng.sync()
        _keep.append(eng)


def workload(n):
    """the interleaved batch of tests 1 and 2: case i under profile i % 4; its oracle results are computed once per n"""
    keep_pool()
    if n not in _workloads:
        inputs = util.corpus_mixed(n, 400, seed=CORPUS_SEED)
        seeds, ids = seeds_of(n), np.arange(n, dtype=np.uint32) % 4
        want, wst, wdr, _ = oracle(inputs, seeds, ids, PROFILES)
        assert not ((wst == 2) | (wst == 3)).any(), "pick other constants: the oracle itself reports an engine-only status"
        _workloads[n] = dict(inputs=inputs, seeds=seeds, ids=ids, want=want, wst=wst, wdr=wdr)
    return _workloads[n]


def new_engine(flags=0, profiles=PROFILES, **conf):
    """a context configured with profiles[0] that knows profiles[1:] under the ids 1 .."""
    eng = ea.Engine(0)
    m, p, b = profiles[0]
    eng.configure(mutations=m, patterns=p, blockscale=b, max_case_bytes=MCB, flags=flags, **conf)
    assert eng.profile_count() == 1
    got = [eng.profile_add(*pr) for pr in profiles]
    assert got == list(range(len(profiles))), got
    return eng


def run_calls(eng, inputs, seeds, ids=None):
    data, off = po.pack(list(inputs))
    eng.upload_corpus(data, off)
    eng.fuzz_calls(seeds, ids)
    outs, st = eng.download()
    dr, lm = eng.diag()
    return outs, [int(x) for x in st], [int(x) for x in dr], [int(x) for x in lm]


def against_oracle(label, got, want, wst, wdr):
    """status, bytes, and draws where the status is 0; a case is left out only when either side reports 2 or 3, at most 3 % of them"""
    outs, st, dr, _ = got
    n = len(outs)
    cmp = [i for i in range(n) if st[i] not in (2, 3) and int(wst[i]) not in (2, 3)]
    bad = [i for i in cmp if st[i] != int(wst[i]) or outs[i] != want[i] or (st[i] == 0 and dr[i] != int(wdr[i]))]
    print("%s: %d cases, %d left out (status 2 / 3), %d differ" % (label, n, n - len(cmp), len(bad)))
    assert n - len(cmp) <= LEFT_OUT_CAP * n, (label, [(i, st[i], int(wst[i])) for i in range(n) if i not in cmp][:10])
    assert not bad, "%s: cases differ: %s" % (label, [(i, st[i], int(wst[i]), len(outs[i]), len(want[i])) for i in bad[:10]])
    return len(cmp)


def mixed_launch(n):
    """ONE fuzz_calls(seeds, profiles) over the interleaved batch (kept: test 2 compares with it)"""
    if n not in _mixed:
        w = workload(n)
        eng = new_engine()
        _mixed[n] = run_calls(eng, w["inputs"], w["seeds"], w["ids"])
        eng.close()
    return _mixed[n]


def parity(n):
    """1. parity with the oracle, profiles interleaved"""
    w = workload(n)
    return against_oracle("interleaved profiles", mixed_launch(n), w["want"], w["wst"], w["wdr"])


def alone(n):
    """2. a profiled batch equals each profile alone, engine against engine: nothing is left out"""
    w, mixed = workload(n), mixed_launch(n)
    inputs, seeds = w["inputs"], w["seeds"]
    eng = ea.Engine(0)
    p3_all = None
    for k, (m, p, b) in enumerate(PROFILES):
        eng.configure(mutations=m, patterns=p, blockscale=b, max_case_bytes=MCB)
        idx = [i for i in range(n) if i % 4 == k]
        got = run_calls(eng, [inputs[i] for i in idx], seeds[idx])
        for q in range(4):                                          # statuses, bytes, draws, last-mutator ids
            assert got[q] == [mixed[q][i] for i in idx], ("profile %d alone" % k, "field %d" % q)
        if k == 3:
            p3_all = run_calls(eng, inputs, seeds)
    eng.close()
    eng = new_engine()
    assert run_calls(eng, inputs, seeds, np.full(n, 3, dtype=np.uint32)) == p3_all, "all ids 3 (the last id) against profile 3 alone"
    assert run_calls(eng, inputs, seeds, np.zeros(n, dtype=np.uint32)) == run_calls(eng, inputs, seeds), "all ids 0 against plain fuzz_calls"
    eng.close()
    return n


def first_occurrences(cases, status):
    seen, out = {}, []
    for i, (b, s) in enumerate(zip(cases, status)):
        out.append(seen.setdefault(b, i) if s == 0 else i)
    return out


def shapes(n):
    """3. shapes where the table indexing can go wrong: batch sizes and table sizes"""
    wl = workload(n)
    inputs, seeds = wl["inputs"], wl["seeds"]
    more = util.corpus_mixed(65, 400, seed=CORPUS_SEED + 1)
    seeds65 = seeds_of(65)
    eng = new_engine()
    # n = 1 with profile 3
    one = run_calls(eng, inputs[5:6], seeds[5:6], [3])
    against_oracle("n = 1, profile 3", one, *oracle(inputs[5:6], seeds[5:6], [3], PROFILES)[:3])
    # n = 65, the id changes at case 64
    ids = np.array([1] * 64 + [2], dtype=np.uint32)
    against_oracle("n = 65, id changes at case 64", run_calls(eng, more, seeds65, ids), *oracle(more, seeds65, ids, PROFILES)[:3])
    # one mutator and one pattern; every GPU mutator (nsel at its maximum) under a work budget
    profs = PROFILES + [("bd", "od", 1.0), (",".join(ea.gpu_mutators()), "od,nd,bu", 1.0)]
    assert eng.profile_add(*profs[4]) == 4 and eng.profile_add(*profs[5]) == 5
    ids = np.array([4, 0] * 8, dtype=np.uint32)
    against_oracle("profile bd / od", run_calls(eng, inputs[:16], seeds[:16], ids), *oracle(inputs[:16], seeds[:16], ids, profs)[:3])
    eng.close()
    eng = new_engine(profiles=profs, max_case_work=8 << 20)
    assert len(ea.gpu_mutators()) == len(ea.mutator_table())
    ids = np.array([5, 5, 5, 0] * 4, dtype=np.uint32)
    against_oracle("every GPU mutator", run_calls(eng, inputs[:16], seeds[:16], ids),
                   *oracle(inputs[:16], seeds[:16], ids, profs, max_case_work=8 << 20)[:3])
    eng.close()
    return True


def shapes_flags(n):
    """3. (continued) the flags that change what happens after a case, and the uniqueness filter, over a profiled batch"""
    wl = workload(n)
    inputs, seeds = wl["inputs"], wl["seeds"]
    # EH_FLAG_ORDERED_OUTPUT
    m = min(n, 64)
    eng = new_engine(flags=engine.EH_FLAG_ORDERED_OUTPUT)
    got = run_calls(eng, wl["inputs"][:m], wl["seeds"][:m], wl["ids"][:m])
    against_oracle("ordered output", got, wl["want"][:m], wl["wst"][:m], wl["wdr"][:m])
    eng.close()
    # EH_FLAG_META_TRACE: the trace text of one case per profile
    eng = new_engine(flags=engine.EH_FLAG_META_TRACE)
    got = run_calls(eng, wl["inputs"][:m], wl["seeds"][:m], wl["ids"][:m])
    _, tst, _, lines = oracle(wl["inputs"][:m], wl["seeds"][:m], wl["ids"][:m], PROFILES, trace="full")
    for k in range(4):
        i = next(i for i in range(k, m, 4) if got[1][i] == 0 and tst[i] == 0)
        assert got[0][i] == wl["want"][i]
        assert util.meta_matches(eng, i, lines[i]), "profile %d case %d: engine %r oracle %r" % (k, i, eng.meta_terms(i)[0][:12], lines[i][:300])
    eng.close()
    # Engine.unique() over a profiled batch: few distinct (input, seed, profile) triples, so the batch repeats itself
    eng = new_engine()
    rep_in = [inputs[i % 3] for i in range(m)]
    rep_seeds = np.array([seeds[3 + i % 2] for i in range(m)], dtype=np.int64)
    rep_ids = np.array([(i // 6) % 4 for i in range(m)], dtype=np.uint32)
    outs, st, _, _ = run_calls(eng, rep_in, rep_seeds, rep_ids)
    first, n_unique, _ = eng.unique()
    first = [int(f) for f in first]
    assert all(outs[f] == outs[i] for i, f in enumerate(first)), "first_of points at a case with other bytes"
    assert first == first_occurrences(outs, st) and n_unique < sum(1 for s in st if s == 0), (n_unique, m)
    eng.close()
    return True


def coalescer(nreq):
    """4. four threads submit under their own profile ids; a fifth profile is added between submits while a batch is in flight; one
    pending and one in-flight ticket are cancelled; every other ticket, polled in random order, gets the bytes of test 1's rule"""
    inputs = util.corpus_mixed(nreq, 400, seed=CORPUS_SEED)
    seeds = seeds_of(nreq)
    profs = PROFILES + [FIFTH]
    tail = 8                                                         # requests the main thread submits itself, after the threads
    per = (nreq - tail) // 4
    owner = [i // per for i in range(4 * per)] + [2, 2] + [4 if j % 2 == 0 else 2 for j in range(nreq - 4 * per - 2)]   # thread t = profile t; the tail: 2 and the fifth
    want, wst, _, _ = oracle(inputs, seeds, owner, profs)
    eng = new_engine()
    eng.coalesce_limits(64, 1 << 20)
    tickets, errors = {}, []

    def client(t):
        try:
            for i in range(t * per, (t + 1) * per):
                tickets[i] = eng.submit(inputs[i], tuple(int(x) for x in seeds[i]), profile=t)
        except Exception as ex:                                      # noqa: BLE001 - reported by the main thread
            errors.append((t, repr(ex)))

    ts = [threading.Thread(target=client, args=(t,)) for t in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errors, errors[:3]
    rest = list(range(4 * per, nreq))
    # a pending ticket is cancelled
    i0 = rest.pop(0)
    t0 = eng.submit(inputs[i0], tuple(int(x) for x in seeds[i0]), profile=owner[i0])
    assert eng.poll(t0) is None                                      # EH_E_AGAIN: not launched yet
    eng.cancel(t0)
    # what is pending goes into flight; the fifth profile arrives while it is there, between two submits
    i1 = rest.pop(0)
    tickets[i1] = eng.submit(inputs[i1], tuple(int(x) for x in seeds[i1]), profile=owner[i1])
    eng.flush()
    assert eng.profile_count() == 4
    fifth = eng.profile_add(*FIFTH)
    assert fifth == 4 and eng.profile_count() == 5
    for i in rest:
        tickets[i] = eng.submit(inputs[i], tuple(int(x) for x in seeds[i]), profile=owner[i])
    eng.cancel(tickets[i1])                                          # in flight: dropped when its batch is collected
    eng.flush()
    cancelled = {i0: t0, i1: tickets.pop(i1)}
    order = np.random.Generator(np.random.PCG64(4)).permutation(sorted(tickets))
    left_out = 0
    for i in order:
        r = eng.poll(tickets[int(i)])
        assert r is not None, ("never launched", int(i))
        if r[0] in (2, 3) or int(wst[i]) in (2, 3):
            left_out += 1
            continue
        assert r == (int(wst[i]), want[i]), ("request %d under profile %d" % (i, owner[i]), r[0], int(wst[i]), len(r[1]), len(want[i]))
    assert left_out <= LEFT_OUT_CAP * nreq, left_out
    for t in cancelled.values():
        assert code(eng.poll, t) == -1                               # EH_E_INVALID: the ticket is gone
    eng.close()
    print("coalescer: %d requests, %d left out" % (len(order), left_out))
    return len(order)


def interning_limits_errors():
    """5. interning, limits, errors"""
    w = workload(64)
    inputs, seeds = w["inputs"][:8], w["seeds"][:8]
    eng = ea.Engine(0)
    assert code(eng.profile_add, "bd") == -5 and eng.profile_count() == 0                  # EH_E_STATE: not configured
    eng.close()
    eng = new_engine()
    assert eng.profile_add(*PROFILES[2]) == 2 and eng.profile_add(*PROFILES[2]) == 2       # the same strings, the same id
    a = eng.profile_add("bd,bf", "od")
    assert a == 4 and eng.profile_add("bd=1,bf=1", "od=1") == a and eng.profile_add("bf,bd", "od", 0) == a
    assert eng.profile_add(*PROFILES[0]) == 0 and eng.profile_add(PROFILES[0][0], PROFILES[0][1], 0) == 0   # the configured one is id 0
    assert eng.profile_add("bd,bf", "od", 1.5) == 5 and eng.profile_count() == 6
    for bad, kw in (("nosuch", {}), ("bd=x", {}), ("bd", {"patterns": "zz"}), ("bd", {"patterns": ""})):
        try:
            eng.profile_add(bad, **kw)
            raise AssertionError("accepted " + bad)
        except EngineError as e:
            assert e.code == -1 and len(str(e)) > 25, (bad, str(e))                            # EH_E_INVALID with a text
    assert eng.profile_count() == 6
    # an id >= count: nothing is queued, nothing is launched
    before = run_calls(eng, inputs, seeds, np.array([5] * 8, dtype=np.uint32))
    assert code(eng.submit, b"request", (1, 2, 3), 6) == -1
    eng.flush()
    assert code(eng.fuzz_calls, seeds, np.array([0, 1, 2, 3, 4, 5, 6, 0], dtype=np.uint32)) == -1
    outs, st = eng.download()
    assert (outs, [int(x) for x in st]) == (before[0], before[1]) and code(eng.fuzz_calls, seeds) == 0
    # eh_configure drops all profiles
    eng.configure(mutations="bd", patterns="od", max_case_bytes=MCB)
    assert eng.profile_count() == 1 and code(eng.fuzz_calls, seeds, np.array([1] * 8, dtype=np.uint32)) == -1
    assert code(eng.submit, b"request", (1, 2, 3), 1) == -1 and eng.profile_add("bd", "od") == 0
    # 1024 distinct profiles, and the 1025th
    for k in range(2, engine.MAX_PROFILES + 1):
        assert eng.profile_add("bd=%d" % k, "od") == k - 1
    assert eng.profile_count() == engine.MAX_PROFILES == 1024
    assert code(eng.profile_add, "bd=5000", "od") == -4 and eng.profile_count() == 1024    # EH_E_NOMEM
    assert eng.profile_add("bd=1024", "od") == 1023 and eng.profile_add("bd=77", "od") == 76   # known ones are still found
    ids = np.full(8, 1023, dtype=np.uint32)
    against_oracle("profile 1023", run_calls(eng, inputs, seeds, ids), *oracle(inputs, seeds, [0] * 8, [("bd=1024", "od", 1.0)])[:3])
    eng.close()
    return True


def api_requests():
    """6. api.fuzz_requests = api.fuzz(data, request_opts) one by one"""
    w = workload(64)
    inputs, seeds = w["inputs"][:32], w["seeds"][:32]
    opts = {"mutations": PROFILES[0][0], "patterns": PROFILES[0][1], "seed": (11, 12, 13), "max_case_bytes": MCB}
    kinds = [{}, {"mutations": PROFILES[1][0], "patterns": PROFILES[1][1], "blockscale": 0.5},
             {"mutations": [("sr", 1), ("sd", 2), ("tr2", 1)], "blockscale": 2.0}, {"patterns": "nd=3,bu"},
             {"mutations": PROFILES[3][0], "patterns": [("bu", 1), ("nu", 1), ("co", 2)], "blockscale": 0.1}]
    requests = []
    for i in range(32):
        ro = dict(kinds[i % len(kinds)])
        if i % 3:
            ro["seed"] = tuple(int(x) for x in seeds[i])
        requests.append((inputs[i], ro))
    got = api.fuzz_requests(requests, opts)
    outs, status = api.fuzz_requests(requests, opts, return_status=True)
    assert len(got) == 32 and [o if s == 0 and o else [] for o, s in zip(outs, status)] == got
    for e in api._engines.values():                                  # a fresh engine for the one-by-one calls
        e.close()
    api._engines.clear()
    assert len(set(bytes(g) for g in got if g != [])) > 16
    for i, (d, ro) in enumerate(requests):
        assert api.fuzz(d, dict(opts, **ro)) == got[i], ("request %d" % i, ro)
    for bad in ((requests[:3] + [(b"abc", {"sequence_muta": True})], opts), (requests[:3], dict(opts, sequence_muta=True))):
        try:
            api.fuzz_requests(*bad)
            raise AssertionError("sequence_muta accepted")
        except api.Unsupported as e:
            assert e.keys == ["sequence_muta"]
    return True


def run(n, nreq):
    return (parity(n), alone(n), shapes(n), shapes_flags(n), coalescer(nreq), interning_limits_errors(), api_requests())


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    print("profiles ok: %s" % (run(n, 300 if n >= 256 else 64),))
