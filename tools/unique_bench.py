#!/usr/bin/env python3
"""What the uniqueness filter (csrc/eh_unique.h) costs and what it saves, on one batch of the bench workload's shape at a size
that runs in seconds: synth.mixed, 8192 cases x 4 KiB, the default mutator table, patterns od,nd,bu (bench.py's defaults).

  python tools/unique_bench.py [--cases 8192] [--size 4096] [--repeats 3] [--out profiles/unique_bench.json]

Records the output bytes, the mutate kernel's milliseconds (eh_last_kernel_ms), the milliseconds of digest + dedup (HIP events
around eh_result_unique's launches, recorded through torch on the null stream the batch runs on; the wall clock of the call
besides, which adds one stream synchronisation and a 16-byte copy) and the rate over the output bytes, the duplicate share by
cases and by bytes, and - each into page-locked memory - the wall time of the full eh_result_download against eh_result_unique +
eh_result_download_select of the unique cases.  The baseline of the second number is the first, from the same run."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

try:                                    # torch first when both share a process
    import torch
    HAVE_EVENTS = torch.cuda.is_available()
except Exception:                       # noqa: BLE001 - the wall clock remains
    HAVE_EVENTS = False
import erlamsa_amd as ea
from erlamsa_amd import synth
from erlamsa_amd.engine import HostBuffer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=8192)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unique_bench.json"))
    args = ap.parse_args()
    n = args.cases
    data, off = synth.as_arena(synth.mixed(n, args.size))
    eng = ea.Engine(0)
    eng.configure(patterns="od,nd,bu", max_case_bytes=4 << 20, max_slots=1024)
    eng.upload_corpus(data, off)
    runs = []
    hbuf = None
    for it in range(args.repeats):
        eng.fuzz_batch(seed=(1, 2, 3), first_case=1 + it * n)
        eng.sync()
        _, total, _ = eng.totals()
        if hbuf is None or hbuf.size < total:
            hbuf = HostBuffer(total + (total >> 2) + 4096)
        r = {"out_bytes": int(total), "mutate_ms": eng.kernel_ms()}
        # digest + dedup: compute only (no array comes back)
        if HAVE_EVENTS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        t0 = time.perf_counter()
        nu, nb = ea.engine.C.c_uint64(), ea.engine.C.c_uint64()
        eng._chk(eng.lib.eh_result_unique(eng.h, None, ea.engine.C.byref(nu), ea.engine.C.byref(nb)))
        t1 = time.perf_counter()
        if HAVE_EVENTS:
            e1.record(); e1.synchronize()
            r["filter_ms_events"] = e0.elapsed_time(e1)
        r["filter_ms_wall"] = (t1 - t0) * 1e3
        ms = r.get("filter_ms_events", r["filter_ms_wall"])
        r["filter_GBps"] = total / (ms * 1e-3) / 1e9
        status = eng.status()
        ok = int((status == 0).sum())
        lens = eng.lens()
        ok_bytes = int(lens[status == 0].sum())
        r.update({"ok_cases": ok, "unique_cases": int(nu.value), "unique_bytes": int(nb.value),
                  "duplicate_share_cases": 1 - nu.value / max(ok, 1), "duplicate_share_bytes": 1 - nb.value / max(ok_bytes, 1)})
        # download, both ways, into page-locked memory
        t0 = time.perf_counter()
        eng.download_into(hbuf.ptr, hbuf.size)
        t1 = time.perf_counter()
        r["download_full_ms"] = (t1 - t0) * 1e3
        eng.fuzz_batch(seed=(1, 2, 3), first_case=1 + it * n)          # the same batch again: nothing of the filter is cached
        eng.sync()
        t0 = time.perf_counter()
        first, _, _ = eng.unique()
        idx = np.flatnonzero((first == np.arange(n, dtype=np.uint64)) & (status == 0))
        o = eng.download_select_into(idx, hbuf.ptr, hbuf.size)
        t1 = time.perf_counter()
        assert int(o[-1]) == nb.value
        r["unique_plus_select_ms"] = (t1 - t0) * 1e3
        r["download_saving"] = 1 - r["unique_plus_select_ms"] / r["download_full_ms"]
        runs.append(r)
        print(json.dumps(r), flush=True)
    res = {"workload": "synth.mixed %d x %d B, default mutators, patterns od,nd,bu, one context, null stream" % (n, args.size),
           "command": "python tools/unique_bench.py --cases %d --size %d --repeats %d" % (n, args.size, args.repeats),
           "filter_timer": "HIP events" if HAVE_EVENTS else "wall clock", "piece_bytes": ea.engine.UNIQUE_PIECE_BYTES, "runs": runs}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
