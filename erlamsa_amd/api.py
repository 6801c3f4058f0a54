"""Option-map level API mirroring erlamsa_main:fuzzer/1 and erlamsa_app:fuzz/1,2.

Option keys are the reference's Dict keys (erlamsa_main.erl:127-163):
  seed        {A,B,C} tuple                      (default: os.urandom, like gen_urandom_seed/0)
  mutations   [(name, pri)] or "-m" string       (default erlamsa_mutations:default/1)
  patterns    [(name, pri)] or "-p" string       (default erlamsa_patterns:default/0)
  generators  [(name, pri)]                      (default: what paths=[direct] leaves: direct=500, random=1)
  n           number of cases                    (default 1)
  input       bytes                              (paths = [direct])
  blockscale  float
  skip        cases numbered <= skip are computed but dropped (erlamsa_main.erl:161,191-196)
  unique      (not the reference's: radamsa's --hash) duplicates are found on the device and only one copy of every distinct output
              is downloaded; fuzzer/1 returns the distinct results in first-occurrence order
  fresh       (not the reference's: radamsa's --checksums N) an int, the capacity of a seen set that the engine of the device keeps
              across calls (made on first use, kept while the capacity asked for stays the same): outputs that repeat an earlier
              case of the batch OR an output of an earlier batch are dropped on the device and never downloaded; fuzzer/1 returns
              only results it has never returned before (cases that `skip` drops count as returned).  Takes precedence over
              `unique`.  Once more distinct outputs than the capacity have gone by, the surplus is not remembered.
Only `paths => [direct]`, `output => return` is served by the GPU path.  Keys the reference honours and a batch
on the GPU cannot - external_mutations (custom mutator funs appended to the table, erlamsa_main.erl:128), external_post (a
post-processor applied per written block, :159), sequence_muta (:223-235) - raise Unsupported: the caller routes that run to
the BEAM path instead of getting a run WITHOUT what it asked for (erlang/src/erlamsa_hip.erl host_only/1 is the same rule).
"""
import os

import numpy as np

from .engine import CASE_OK, SEEN_FRESH, Engine, mutator_table, pattern_table

_engines = {}


def _engine(device=0):
    e = _engines.get(device)
    if e is None:
        e = _engines[device] = Engine(device)
    return e


def default_mutations():
    """erlamsa_mutations:default/1 -> [(name, pri)] (erlamsa_mutations.erl:1358-1359)"""
    return [(n, p) for n, p, _ in mutator_table()]


def default_patterns():
    """erlamsa_patterns:default/0 (erlamsa_patterns.erl:407-408)"""
    return [(n, p) for n, p, _ in pattern_table()]


def actions_to_string(lst):
    if lst is None or isinstance(lst, str):
        return lst
    return ",".join("%s=%d" % (n, p) for n, p in lst)


def pack_corpus(inputs):
    """list[bytes] -> (uint8 arena, uint64 off[n+1])  — the packed offset/length arena"""
    off = np.zeros(len(inputs) + 1, dtype=np.uint64)
    if inputs:
        off[1:] = np.cumsum([len(b) for b in inputs], dtype=np.uint64)
    joined = b"".join(inputs)
    data = np.frombuffer(joined, dtype=np.uint8).copy() if joined else np.zeros(1, dtype=np.uint8)
    return data, off


def _seed_of(opts):
    s = opts.get("seed")
    if s is None:  # gen_urandom_seed/0 erlamsa_rnd.erl:50-62: three 16-bit values
        raw = os.urandom(6)
        s = tuple(int.from_bytes(raw[2 * i:2 * i + 2], "big") for i in range(3))
    return tuple(int(x) for x in s)


def _configure(eng, opts):
    eng.configure(mutations=actions_to_string(opts.get("mutations")), patterns=actions_to_string(opts.get("patterns")),
                  generators=actions_to_string(opts.get("generators")), blockscale=float(opts.get("blockscale", 1.0)),
                  ssrf_host=opts.get("ssrf_host"), ssrf_port=int(opts.get("ssrf_port", 0)),
                  max_case_bytes=int(opts.get("max_case_bytes", 0)), out_capacity=int(opts.get("out_capacity", 0)),
                  max_slots=int(opts.get("max_slots", 0)), max_case_work=int(opts.get("max_case_work", 0)))


class Unsupported(ValueError):
    """The option map carries keys only erlamsa_main:fuzzer/1 on BEAM can honour: `.keys` (the shim's {error, {unsupported, Keys}})."""

    def __init__(self, keys):
        super().__init__("not served by the GPU path, route this run to erlamsa_main:fuzzer/1: %s" % ", ".join(keys))
        self.keys = keys


def host_only(opts):
    """keys of the Dict that are set and need the BEAM (erlamsa_hip:host_only/1)"""
    keys = [k for k in ("external_mutations", "external_post") if opts.get(k) is not None]
    if opts.get("sequence_muta"):
        keys.append("sequence_muta")
    return keys


def fuzz_batch(inputs, opts=None, return_status=False, device=0):
    """Case I (1-based) of ONE fuzzer/1 run mutates inputs[I-1].  -> list[bytes] (and statuses).
    With opts["unique"] and return_status: (outs, status, first_of).  With opts["fresh"]: the cases that are not fresh come back as b"",
    and with return_status: (outs, status, cls), cls as eh_result_seen gives it."""
    opts = dict(opts or {})
    if host_only(opts):
        raise Unsupported(host_only(opts))
    eng = _engine(device)
    _configure(eng, opts)
    _seen_set(eng, opts)
    data, off = pack_corpus(list(inputs))
    eng.upload_corpus(data, off)
    eng.fuzz_batch(seed=_seed_of(opts), first_case=int(opts.get("first_case", 1)), n=len(inputs))
    return _batch_results(eng, opts, return_status)


def _seen_set(eng, opts):
    """opts["fresh"]: the engine keeps a seen set of that capacity (made on first use, kept while the capacity stays the same)"""
    if opts.get("fresh"):
        capacity = int(opts["fresh"])
        if capacity < 1:
            raise ValueError("fresh: the capacity of the seen set, a positive int")
        if eng.seen_count()[1] != capacity:
            eng.seen_reserve(capacity)


def _batch_results(eng, opts, return_status):
    """what fuzz_batch returns for the engine's last batch"""
    if opts.get("fresh"):
        # only the cases that are neither a repeat inside the batch nor an output of an earlier batch cross PCIe
        cls, _, _ = eng.result_seen(commit=True)
        status = eng.status()
        idx = np.flatnonzero(cls == SEEN_FRESH)
        outs = [b""] * len(cls)
        for i, o in zip(idx.tolist(), eng.download_select(idx)):
            outs[i] = o
        return (outs, status, cls) if return_status else outs
    if not opts.get("unique"):
        outs, status = eng.download()
        return (outs, status) if return_status else outs
    # one copy of every distinct output crosses PCIe; the other cases share its bytes object
    first_of, _, _ = eng.unique()
    status = eng.status()
    reps = np.flatnonzero(first_of == np.arange(len(first_of), dtype=np.uint64))
    got = dict(zip(reps.tolist(), eng.download_select(reps)))
    outs = [got[int(f)] for f in first_of]
    return (outs, status, first_of) if return_status else outs


def fuzz_generations(inputs, opts=None, generations=1, keep="all", return_status=False, device=0):
    """A generational campaign on the device: generation g is ONE batch over the whole current corpus, and what it keeps becomes the
    corpus of generation g + 1 without crossing PCIe (Engine.corpus_promote / corpus_promote_fresh, replace mode).  Case numbers
    continue where the previous generation stopped, as one fuzzer/1 run would count them.
      keep="all"    every EH_CASE_OK case of non-zero length, in case order: what record_result/2 keeps (erlamsa_main.erl:120-122)
      keep="fresh"  the cases no earlier case of the campaign's seen set has produced (opts["fresh"]: the set's capacity), none longer
                    than opts["max_entry_bytes"] (0 or absent: no limit)
    -> what fuzz_batch returns for the LAST generation that ran (with return_status the statuses, and the classes with "fresh"); the
    campaign stops early when a generation promotes nothing.  Cases that stopped at an engine limit are never promoted."""
    opts = dict(opts or {})
    if host_only(opts):
        raise Unsupported(host_only(opts))
    if keep not in ("all", "fresh"):
        raise ValueError("keep: 'all' or 'fresh'")
    if keep == "fresh" and not opts.get("fresh"):
        raise ValueError("keep='fresh' needs opts['fresh'], the capacity of the seen set")
    if int(generations) < 1:
        raise ValueError("generations: a positive int")
    eng = _engine(device)
    _configure(eng, opts)
    _seen_set(eng, opts)
    data, off = pack_corpus(list(inputs))
    eng.upload_corpus(data, off)
    seed, first = _seed_of(opts), int(opts.get("first_case", 1))
    for g in range(int(generations)):
        n = eng.n_corpus
        eng.fuzz_batch(seed=seed, first_case=first, n=n)
        first += n
        if keep == "fresh":
            taken, _ = eng.corpus_promote_fresh(max_entry_bytes=int(opts.get("max_entry_bytes", 0)))
        else:
            taken, _ = eng.corpus_promote(np.flatnonzero((eng.status() == CASE_OK) & (eng.lens() > 0)))
        if not taken:
            break
    return _batch_results(eng, opts, return_status)


class EngineLimit(RuntimeError):
    """Cases of a fuzzer() call stopped at an engine limit the reference does not have (statuses 2 overflow,
    3 unsupported, 4 arena full, 5 work budget): `.cases` = [(index, status)], `.results` = what the other cases gave."""

    def __init__(self, cases, results):
        super().__init__("%d case(s) stopped at an engine limit: %s" % (len(cases), cases[:8]))
        self.cases, self.results = cases, results


def fuzz_requests(requests, opts=None, return_status=False, device=0):
    """N erlamsa_app:fuzz(Data, RequestOpts) calls in ONE launch: requests = [(data, request_opts)].  What erlamsa_esi reads from
    every HTTP request (erlamsa_esi.erl:30-68) - seed, mutations, patterns, blockscale - comes from the request's own options and
    falls back to `opts`; every other key (generators, ssrf_*, max_case_*, ...) comes from `opts`.  The requests' option sets become
    option profiles of the engine (Engine.profile_add), their cases run side by side.
    -> list with, per request, what fuzz/2 returns (the mutated binary, [] when the result is empty); with return_status the raw
    outputs and the statuses, as fuzz_batch does.  A request that stopped at an engine limit raises EngineLimit unless
    opts["on_engine_limit"] == "skip" or return_status is set."""
    opts = dict(opts or {})
    requests = [(bytes(d), dict(ro or {})) for d, ro in requests]
    keys = host_only(opts)
    for _, ro in requests:
        keys += [k for k in host_only(ro) if k not in keys]
    if keys:
        raise Unsupported(keys)
    eng = _engine(device)
    _configure(eng, opts)
    ids, seeds = [], []
    for _, ro in requests:
        per = {k: ro[k] if k in ro else opts.get(k) for k in ("seed", "mutations", "patterns", "blockscale")}
        ids.append(eng.profile_add(actions_to_string(per["mutations"]), actions_to_string(per["patterns"]),
                                   float(per["blockscale"] if per["blockscale"] is not None else 1.0)))
        seeds.append(_seed_of(per))
    data, off = pack_corpus([d for d, _ in requests])
    eng.upload_corpus(data, off)
    if not requests:
        return ([], np.zeros(0, dtype=np.int32)) if return_status else []
    eng.fuzz_calls(np.array(seeds, dtype=np.int64), np.array(ids, dtype=np.uint32))
    outs, status = eng.download()
    if return_status:
        return outs, status
    limited = [(i, int(s)) for i, s in enumerate(status) if s >= 2]
    res = [o if s == CASE_OK and len(o) > 0 else [] for o, s in zip(outs, status)]
    if limited and opts.get("on_engine_limit", "raise") != "skip":
        raise EngineLimit(limited, res)
    return res


def fuzzer(opts):
    """erlamsa_main:fuzzer/1 for paths=[direct], output=return: the same input N times.
    Like record_result/2 (erlamsa_main.erl:120-122) empty results are dropped (a crashed worker, status 1, gives <<>>).
    A case that stopped at an engine-only limit is never dropped silently: EngineLimit is raised unless
    opts["on_engine_limit"] == "skip" (then the caller reads the statuses through fuzz_batch(return_status=True)).
    opts["unique"]: the distinct results, each where it first occurs among the cases that are kept.
    opts["fresh"]: only the results that no earlier call with the same seen set has returned (and each of them once)."""
    opts = dict(opts)
    if opts.get("paths", ["direct"]) != ["direct"] or opts.get("output", "return") != "return":
        raise ValueError("only paths=[direct], output=return is served by the GPU path")
    if host_only(opts):
        raise Unsupported(host_only(opts))
    n = int(opts.get("n", 1))
    skip, first = int(opts.get("skip", 0)), int(opts.get("first_case", 1))
    got = fuzz_batch([bytes(opts.get("input", b""))] * n, opts, return_status=True, device=int(opts.get("device", 0)))
    outs, status = got[0], got[1]
    fresh = got[2] == SEEN_FRESH if opts.get("fresh") else None  # with a seen set: the device has said which cases are new
    first_of = got[2] if opts.get("unique") and fresh is None else range(n)       # without the filter every case is its own first
    res, limited, seen = [], [], set()
    for i, (o, s) in enumerate(zip(outs, status)):
        if first + i <= skip:                                   # `I =< Skip` (erlamsa_main.erl:191): written to the skip port, which keeps nothing
            continue
        if s == CASE_OK and fresh is not None and not fresh[i]:
            continue
        if s == CASE_OK and len(o) > 0:
            if int(first_of[i]) not in seen:
                seen.add(int(first_of[i]))
                res.append(o)
        elif s >= 2:
            limited.append((i, int(s)))
    if limited and opts.get("on_engine_limit", "raise") != "skip":
        raise EngineLimit(limited, res)
    return res


def fuzz(data, opts=None):
    """erlamsa_app:fuzz/1,2: one case; returns the mutated binary ([] when the result is empty,
    like extract_function/1 on an empty list, erlamsa_utils.erl:96-99)."""
    r = fuzzer(dict(opts or {}, input=bytes(data), n=1))
    return r[0] if r else []
