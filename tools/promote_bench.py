#!/usr/bin/env python3
"""What corpus promotion (csrc/eh_promote.h) buys over the host loop it replaces, on the workload of tools/seen_bench.py: synth.mixed,
8192 cases x 4 KiB, the default mutator table, patterns od,nd,bu, a seen set of 131 072 keys, four generations of one run with seed
(1, 2, 3) - generation g is one batch over the whole corpus generation g - 1 left.

  python tools/promote_bench.py [--cases 8192] [--size 4096] [--generations 4] [--out profiles/promote_bench.json]

Both legs run on the SAME batch of every generation, so that they must leave the same corpus bytes (asserted):
  shared  eh_result_seen(commit): the filter and the set, which both legs need before they can choose
  leg B   the host loop that exists without this: eh_result_download_select of the fresh cases of 1 .. 1 MiB into page-locked memory (the
          selective download packs them back to back: that is the repack), the offsets, eh_corpus_upload
  leg A   eh_corpus_promote_fresh(max_entry_bytes = 1 MiB), replace mode (the batch's classes are cached: no second classification)
Leg B runs first and leg A replaces what B uploaded, from the same results; the next generation runs over A's corpus.  Wall clock around
the calls of the Python binding; "bytes moved" is the kept bytes once per direction (B: device to host and back, A: read and written
in HBM)."""
import argparse
import hashlib
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

MAX_ENTRY = 1 << 20


def corpus_hash(eng):
    data, off = eng.corpus_download()
    return hashlib.sha1(data.tobytes() + off.tobytes()).hexdigest(), len(off) - 1, int(off[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=8192)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--generations", type=int, default=4)
    ap.add_argument("--capacity", type=int, default=131072)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "promote_bench.json"))
    args = ap.parse_args()
    data, off = synth.as_arena(synth.mixed(args.cases, args.size))
    eng = ea.Engine(0)
    eng.configure(patterns="od,nd,bu", max_case_bytes=4 << 20, max_slots=1024)
    eng.upload_corpus(data, off)
    eng.seen_reserve(args.capacity)
    first, runs, hbuf = 1, [], None
    for g in range(args.generations):
        n = eng.n_corpus
        t0 = time.perf_counter()
        eng.fuzz_batch(seed=(1, 2, 3), first_case=first, n=n)
        eng.sync()
        t1 = time.perf_counter()
        first += n
        _, total, _ = eng.totals()
        r = {"generation": g + 1, "cases": n, "in_bytes": int(eng.corpus_size()[1]), "out_bytes": int(total), "batch_ms": (t1 - t0) * 1e3}
        t0 = time.perf_counter()
        cls, nf, nb = eng.result_seen(commit=True)
        t1 = time.perf_counter()
        r["seen_ms"] = (t1 - t0) * 1e3
        status, lens = eng.status(), eng.lens()
        r["cases_by_status"] = np.bincount(status, minlength=6).tolist()
        r["cases_by_class"] = [int((cls == c).sum()) for c in range(4)]
        if hbuf is None or hbuf.size < nb + 4096:
            hbuf = HostBuffer(int(nb) + (int(nb) >> 2) + 4096)
        # leg B: choose on the host, fetch, upload
        t0 = time.perf_counter()
        idx = np.flatnonzero((cls == 0) & (status == 0) & (lens >= 1) & (lens <= MAX_ENTRY))
        o = eng.download_select_into(idx, hbuf.ptr, hbuf.size)
        eng.upload_corpus(hbuf.array[:max(int(o[-1]), 1)], o)
        t1 = time.perf_counter()
        kept, kept_bytes = len(idx), int(o[-1])
        r["leg_b_ms"] = (t1 - t0) * 1e3
        hb = corpus_hash(eng)
        # leg A: the same selection and the copy on the device
        t0 = time.perf_counter()
        taken, taken_bytes = eng.corpus_promote_fresh(max_entry_bytes=MAX_ENTRY)
        t1 = time.perf_counter()
        r["leg_a_ms"] = (t1 - t0) * 1e3
        ha = corpus_hash(eng)
        assert (taken, taken_bytes) == (kept, kept_bytes) and ha == hb, "the legs leave different corpora: %s / %s" % (ha, hb)
        r["kept_cases"], r["kept_bytes"] = kept, kept_bytes
        for leg in ("a", "b"):
            ms = r["leg_%s_ms" % leg]
            r["leg_%s_bytes_moved" % leg] = 2 * kept_bytes
            r["leg_%s_GBps_of_kept_bytes" % leg] = kept_bytes / ms / 1e6 if ms else 0.0
            r["leg_%s_share_of_generation" % leg] = (r["seen_ms"] + ms) / (r["batch_ms"] + r["seen_ms"] + ms)
        r["keys_held"], _, r["keys_dropped"], _ = eng.seen_count()
        runs.append(r)
        print(json.dumps(r), flush=True)
        if not kept:
            break
    res = {"workload": "synth.mixed %d x %d B, default mutators, patterns od,nd,bu, a seen set of %d keys, %d generations of one run, max_entry_bytes %d"
                       % (args.cases, args.size, args.capacity, args.generations, MAX_ENTRY),
           "command": "python tools/promote_bench.py --cases %d --size %d --generations %d" % (args.cases, args.size, args.generations),
           "timer": "wall clock", "runs": runs}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
