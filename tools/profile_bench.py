#!/usr/bin/env python3
"""What option profiles (eh_profile_add / eh_submit_profiled) buy a service whose clients send different -m / -p / -b values:
4096 requests of 400 .. 4096 bytes (synth.mixed rows cut to length), spread evenly over 8 profiles, run

  profiled        as ONE coalesced batch: configure once, profile_add for every request, submit under its id, poll;
  reconfigured    as a service has to without profiles, at its best: the requests sorted by profile, then per profile
                  configure + submit its requests + flush + poll (8 launches);
  arrival order   (the first --arrival requests only) the same service when it takes the requests as they come: a launch whenever
                  the options change, here at every request; against the profiled batch over the same requests.

  python tools/profile_bench.py [--set wide|small] [--requests 4096] [--repeats 3] [--out profiles/profile_bench.json]
                                [--bench-parent v1,v2,v3 --bench-change v1,v2,v3]

Both legs go through the same Python binding (one ctypes call per submit and per poll), run on one context and give the same bytes
(checked).  Written: requests/s of both legs per repeat, their medians and the ratio.  --bench-parent / --bench-change record the
`value` lines of three bench.py runs on the parent commit and on this one next to it (mode 0: what profiles must not slow down)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import erlamsa_amd as ea
from erlamsa_amd import synth

# "wide": with sr (seq_repeat) and tr / tr2 (tree stutter / dup), whose results run to megabytes: 2.2 GB come back for 9 MB of requests,
# and both legs mostly move those.  "small": the same profiles without the three; a request's result stays within a few times its size.
SETS = {"wide": [("bd,bf,bi,sr,sd,num,ld,lr,ab,uw", "od,nd,bu", 1.0), ("num=5,ld,lr2,lis", "od", 0.5),
                 ("sr,sd,sp,snand,srnd,tr2,td", "nd,bu,sk", 2.0), ("uw,ui,ab,ad,len", "bu,nu,co", 0.1),
                 ("bd,bf=3,sr", "od,nd", 1.5), ("bei,bed,ber,br,bi=4", "nd", 1.0), ("lds,lri,ls,lp,lrs", "od,bu", 0.25), ("tr,ts1,ts2,td,num", "od,nd,bu", 4.0)],
        "small": [("bd,bf,bi,sd,num,ld,lr,ab,uw", "od,nd,bu", 1.0), ("num=5,ld,lr2,lis", "od", 0.5),
                  ("sd,sp,snand,srnd,td", "nd,bu,sk", 2.0), ("uw,ui,ab,ad,len", "bu,nu,co", 0.1),
                  ("bd,bf=3,bi", "od,nd", 1.5), ("bei,bed,ber,br,bi=4", "nd", 1.0), ("lds,lri,ls,lp,lrs", "od,bu", 0.25), ("ts1,ts2,td,num", "od,nd,bu", 4.0)]}
PROFILES = SETS["wide"]
CONF = dict(max_case_bytes=8 << 20, max_slots=1024)


def requests_of(n):
    rng = np.random.Generator(np.random.PCG64(7))
    rows = synth.mixed(n, 4096, seed=8)
    lens = rng.integers(400, 4097, size=n)
    seeds = rng.integers(1, 99999, size=(n, 3)).astype(np.int64)
    return [(bytes(rows[i, :int(lens[i])]), tuple(int(x) for x in seeds[i]), i % len(PROFILES)) for i in range(n)]


def profiled(eng, reqs):
    m, p, b = PROFILES[0]
    eng.configure(mutations=m, patterns=p, blockscale=b, **CONF)
    eng.coalesce_limits(len(reqs), 1 << 30)
    tickets = [eng.submit(d, s, eng.profile_add(*PROFILES[k])) for d, s, k in reqs]      # profile_add per request, as a service would
    eng.flush()
    return [eng.poll(t) for t in tickets]


def reconfigured(eng, reqs):
    out = [None] * len(reqs)
    for k, (m, p, b) in enumerate(PROFILES):
        eng.configure(mutations=m, patterns=p, blockscale=b, **CONF)
        eng.coalesce_limits(len(reqs), 1 << 30)
        mine = [i for i, r in enumerate(reqs) if r[2] == k]
        tickets = [eng.submit(reqs[i][0], reqs[i][1]) for i in mine]
        eng.flush()
        for i, t in zip(mine, tickets):
            out[i] = eng.poll(t)
    return out


def arrival_order(eng, reqs):
    """the requests as they arrive (profile i % 8: every request differs from the one before): a service without profiles launches
    what is pending and reconfigures whenever the options change"""
    out, pending, cur = [], [], None

    def drain():
        eng.flush()
        out.extend(eng.poll(t) for t in pending)
        del pending[:]

    for d, s, k in reqs:
        if k != cur:
            drain()
            m, p, b = PROFILES[k]
            eng.configure(mutations=m, patterns=p, blockscale=b, **CONF)
            cur = k
        pending.append(eng.submit(d, s))
    drain()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="wide", choices=sorted(SETS), help="the eight profiles: with (wide) or without (small) the mutators whose results run to megabytes")
    ap.add_argument("--requests", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--arrival", type=int, default=512, help="requests of the arrival-order leg (0 = skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "profile_bench.json"))
    ap.add_argument("--bench-parent", default="")
    ap.add_argument("--bench-change", default="")
    args = ap.parse_args()
    global PROFILES
    PROFILES = SETS[args.set]
    reqs = requests_of(args.requests)
    eng = ea.Engine(0)
    assert profiled(eng, reqs[:64]) == reconfigured(eng, reqs[:64])                    # warm-up: pool, slots, arena
    runs = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        a = profiled(eng, reqs)
        t1 = time.perf_counter()
        b = reconfigured(eng, reqs)
        t2 = time.perf_counter()
        assert a == b, "the two legs gave different bytes"
        runs.append({"profiled_requests_per_s": len(reqs) / (t1 - t0), "reconfigured_requests_per_s": len(reqs) / (t2 - t1),
                     "out_bytes": sum(len(r[1]) for r in a), "statuses": np.bincount([r[0] for r in a], minlength=6).tolist()})
        print(json.dumps(runs[-1]), flush=True)
    arrival = None
    if args.arrival:
        sub = reqs[:args.arrival]
        t0 = time.perf_counter()
        a = profiled(eng, sub)
        t1 = time.perf_counter()
        b = arrival_order(eng, sub)
        t2 = time.perf_counter()
        assert a == b, "the arrival-order leg gave different bytes"
        arrival = {"requests": len(sub), "launches_reconfigured": len(sub), "profiled_requests_per_s": len(sub) / (t1 - t0),
                   "reconfigured_requests_per_s": len(sub) / (t2 - t1), "ratio": (t2 - t1) / (t1 - t0)}
        print(json.dumps(arrival), flush=True)
    eng.close()
    pa = statistics.median(r["profiled_requests_per_s"] for r in runs)
    re = statistics.median(r["reconfigured_requests_per_s"] for r in runs)
    res = {"workload": "%d requests of 400 .. 4096 B (synth.mixed rows cut to length) over %d profiles, one context, Python binding" % (len(reqs), len(PROFILES)),
           "command": "python tools/profile_bench.py --set %s --requests %d --repeats %d" % (args.set, args.requests, args.repeats),
           "profiles": [list(p) for p in PROFILES], "runs": runs,
           "profiled_requests_per_s_median": pa, "reconfigured_requests_per_s_median": re, "ratio": pa / re, "arrival_order": arrival}
    for key, val in (("bench_value_parent", args.bench_parent), ("bench_value_change", args.bench_change)):
        if val:
            res[key] = [float(x) for x in val.split(",")]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("profiled_requests_per_s_median", "reconfigured_requests_per_s_median", "ratio")}))


if __name__ == "__main__":
    main()
