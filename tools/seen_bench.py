#!/usr/bin/env python3
"""What the seen set (csrc/eh_seen.h) finds and what it costs over the batches of ONE run: 8 consecutive batches of the bench
workload's shape at a size that runs in seconds - synth.mixed, 8192 cases x 4 KiB, the default mutator table, patterns od,nd,bu
(bench.py's defaults) - batch k being the cases k * 8192 + 1 .. of the run with seed (1, 2, 3) over the same corpus.

  python tools/seen_bench.py [--cases 8192] [--size 4096] [--batches 8] [--out profiles/seen_bench.json]

Per batch it records the class shares of eh_result_seen by cases and by bytes (fresh, repeat inside the batch, seen in an earlier
batch, not EH_CASE_OK), the wall time of eh_result_unique alone (the filter: digests, duplicates) and of eh_result_seen on top of
it (a lane-per-case lookup, a one-wavefront scan, the append and the insert), and - each into page-locked memory - the wall time of
the full eh_result_download against eh_result_seen + eh_result_download_select of the fresh cases.  The batch is launched twice
with the same case numbers, so that neither way finds anything of the other's cached; the first launch's eh_result_seen does not
commit.  The set is seeded with the corpus (eh_seen_add_corpus)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import erlamsa_amd as ea
from erlamsa_amd import synth
from erlamsa_amd.engine import HostBuffer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=8192)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seen_bench.json"))
    args = ap.parse_args()
    n = args.cases
    data, off = synth.as_arena(synth.mixed(n, args.size))
    eng = ea.Engine(0)
    eng.configure(patterns="od,nd,bu", max_case_bytes=4 << 20, max_slots=1024)
    eng.upload_corpus(data, off)
    eng.seen_reserve(2 * n * args.batches)
    corpus_keys = eng.seen_add_corpus()
    runs = []
    hbuf = None
    for it in range(args.batches):
        eng.fuzz_batch(seed=(1, 2, 3), first_case=1 + it * n)
        eng.sync()
        _, total, _ = eng.totals()
        if hbuf is None or hbuf.size < total:
            hbuf = HostBuffer(total + (total >> 2) + 4096)
        r = {"batch": it + 1, "out_bytes": int(total), "mutate_ms": eng.kernel_ms()}
        # the filter alone, then the set on top of it (no commit: the second launch records)
        t0 = time.perf_counter()
        eng.unique()
        t1 = time.perf_counter()
        cls, nf, nb = eng.result_seen(commit=False)
        t2 = time.perf_counter()
        r["unique_ms"] = (t1 - t0) * 1e3
        r["seen_on_top_ms"] = (t2 - t1) * 1e3
        status = eng.status()
        lens = eng.lens()
        ok = max(int((status == 0).sum()), 1)
        ok_bytes = max(int(lens[status == 0].sum()), 1)
        r["cases_by_status"] = np.bincount(status, minlength=6).tolist()
        r["cases_by_class"] = [int((cls == c).sum()) for c in range(4)]
        r["bytes_by_class"] = [int(lens[cls == c].sum()) for c in range(4)]
        r["share_of_ok_cases"] = [r["cases_by_class"][c] / ok for c in range(3)]
        r["share_of_ok_bytes"] = [r["bytes_by_class"][c] / ok_bytes for c in range(3)]
        assert nf == r["cases_by_class"][0] and nb == r["bytes_by_class"][0]
        t0 = time.perf_counter()
        eng.download_into(hbuf.ptr, hbuf.size)
        t1 = time.perf_counter()
        r["download_full_ms"] = (t1 - t0) * 1e3
        eng.fuzz_batch(seed=(1, 2, 3), first_case=1 + it * n)          # the same batch again: nothing of the filter or the set is cached
        eng.sync()
        t0 = time.perf_counter()
        cls2, nf2, nb2 = eng.result_seen(commit=True)
        idx = np.flatnonzero(cls2 == 0)
        o = eng.download_select_into(idx, hbuf.ptr, hbuf.size)
        t1 = time.perf_counter()
        assert int(o[-1]) == nb2
        # the relaunch has the same case numbers; where its classes differ from the first launch's, the statuses say why
        status2 = eng.status()
        r["relaunch"] = {"cases_by_status": np.bincount(status2, minlength=6).tolist(), "classes_differ": int((cls != cls2).sum()),
                         "statuses_differ": int((status != status2).sum()), "fresh_bytes": int(nb2)}
        r["seen_plus_select_ms"] = (t1 - t0) * 1e3
        r["download_saving"] = 1 - r["seen_plus_select_ms"] / r["download_full_ms"]
        r["keys_held"], _, r["keys_dropped"], _ = eng.seen_count()
        runs.append(r)
        print(json.dumps(r), flush=True)
    res = {"workload": "synth.mixed %d x %d B, default mutators, patterns od,nd,bu, one context, null stream, %d consecutive batches of one run" % (n, args.size, args.batches),
           "command": "python tools/seen_bench.py --cases %d --size %d --batches %d" % (n, args.size, args.batches),
           "timer": "wall clock", "capacity": 2 * n * args.batches, "corpus_keys": corpus_keys, "runs": runs}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
