"""The delimiter matcher of the tree mutators decides 64 runs of TL_S = 32 events at a time, one run per lane, and a walk over the
lanes settles what depended on the stack below a run (csrc/eh_tree.h tree_parse).  Blocks of 1 - 64 KiB aimed at the places where
that can go wrong, under ts1, ts2, tr2, td / od (tr is left out: its stutter overflows by design): the lane batches (default), the
sequential loop alone (EH_FLAG_TREE_NO_LANES) and the oracle must agree on status, length, draw count and SHA-1 of every case, and
every case must end with status 0 - none is skipped.

The same body runs on the CPU wavefront emulator (as a subprocess of this file, ERLAMSA_HIP_LIB = the emulator build) and, marked
gpu, on the device with the product library.  One more emulator test reads the batch counters the emulator build keeps (events
committed by lane batches, batches, batches that committed too little and sent a stretch to the sequential loop).

  ERLAMSA_HIP_LIB=build/liberlamsa_hip_emu.so python tests/test_tree_lanes.py [emu|full|counters]
"""
import hashlib
import os
import random
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "hipemu")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _define(path, name):
    """the value of `#define name` in a source file of the tree: the inputs below follow the build, not a copy of its constants"""
    m = re.search(r"^#define\s+%s\s+(\d+)" % name, open(os.path.join(ROOT, path)).read(), re.M)
    return int(m.group(1))


EH_FLAG_TREE_NO_LANES = _define("include/erlamsa_hip.h", "EH_FLAG_TREE_NO_LANES")
S = _define("erlamsa_amd/csrc/eh_tree.h", "EH_TREE_S")        # events per run; a batch is 64 runs
B = 64 * S
MUTS, PATS, SEED = "ts1,ts2,tr2,td", "od", (11, 22, 33)
OPEN, CLOSE = b"([<{", b")]>}"


def _nested(rnd, nev, maxdepth=6, fill=0.3):
    """exactly nev bracket events (no quotes): a random well-nested text, whatever is still open at the end stays unclosed"""
    out, st = bytearray(), []
    for _ in range(nev):
        if st and (len(st) >= maxdepth or rnd.random() < 0.5):
            out.append(CLOSE[st.pop()])
        else:
            k = rnd.randrange(4); st.append(k); out.append(OPEN[k])
        if rnd.random() < fill:
            out += bytes(rnd.choice(b"abc 12") for _ in range(rnd.randint(1, 3)))
    return bytes(out)


def _mix(rnd, nev, quotes):
    """nev random events: openers, closers that may match nothing, a share of quotes"""
    out = bytearray()
    for _ in range(nev):
        r = rnd.random()
        if r < quotes: out.append(rnd.choice(b"\"'"))
        elif r < quotes + (1 - quotes) * 0.5: out.append(rnd.choice(OPEN))
        else: out.append(rnd.choice(CLOSE))
        if rnd.random() < 0.25: out += b"xy"[:rnd.randint(1, 2)]
    return bytes(out)


def _chain(rnd, depth):
    ks = [rnd.randrange(4) for _ in range(depth)]
    return bytes(OPEN[k] for k in ks), bytes(CLOSE[k] for k in reversed(ks))


def inputs(full):
    """(name, block): `full` adds the long blocks (up to 64 KiB) the emulator would take minutes for, and runs every block as four
    cases (a case's number is part of its seed: other mutators, other nodes picked)"""
    rnd = random.Random(7)
    pad = b"plain text without any delimiter, " * 31                 # 1 KiB and more for the blocks with few events
    out = []
    # event counts around one batch, and fewer than 64 events
    for n in (B - 1, B, B + 1):
        out.append(("events_%d" % n, _nested(rnd, n)))
    out.append(("events_40", pad + _nested(rnd, 40) + pad))
    # a node opened in one run and closed in a later one / in the next batch
    out.append(("node_across_runs", b"".join(b"(" + b"[a]" * rnd.randint(10, 40) + b")" for _ in range(30))))
    out.append(("node_across_batches", b"{" + b"(a)<b>" * 600 + b"}" + b"[" + b"(c)" * 200 + b"]"))
    # a quote as the first event of a run (event S, 3 S, ... : the units are 2 S events long): the outer top waits for it / does not
    body = b"(a)" * ((S - 2) // 2) + b"]"                              # S - 1 events that leave the stack as it was
    out.append(("quote_first_waiting", (b'"' + body + b'"' + b"[x]" * ((S - 2) // 2) + b"}") * 12 + _nested(rnd, 300)))
    out.append(("quote_first_not_waiting", (b"<" + body + b'"' + b"[x]" * ((S - 4) // 2) + b"]" + b'"' + b">") * 12 + _nested(rnd, 300)))
    out.append(("quote_first_later_batch", b"(a)" * (B // 2) + b"'" + body + b"'" + b"(b)" * 200))
    # alternating quotes (every one is pushed), and quotes only (push, close, push, ...): stops everywhere, the fallback's case
    out.append(("quotes_alternating", b"\"'" * 700 + b"(a)" * 50))
    out.append(("quotes_only", (b'"' * 1500 + b"q" + b"'" * 1501)))
    out.append(("quotes_around_brackets", b"".join(b'"' + b"(a[b]c)" * rnd.randint(1, 30) + b'" ' for _ in range(80))))
    # stray closers at local depth 0 that match / do not match the outer top
    out.append(("stray_closers", b"".join(b"(" + b"[a]" * rnd.randint(5, 20) + rnd.choice([b")", b"}", b"]", b">)", b"})]"]) for _ in range(150))))
    # unclosed openers that block everything below them
    out.append(("unclosed_block", b"(a)" * 300 + b"{" + b"[b]" * 300 + b"<" + b"(c)" * 200 + b")" * 7 + b"}" + b"]" * 5 + b"(d)" * 100))
    # local nesting of S + 1, real nesting of 65, 96 and 129 (spill and refill of the lane-register stack)
    for d in (S + 1, 65, 96, 129):
        blk = bytearray()
        for _ in range(max(2, 700 // (2 * d) + 1)):
            o, c = _chain(rnd, d)
            blk += o + b"k" + c[:rnd.randint(d // 2, d)] + b" "
        o, c = _chain(rnd, d)
        out.append(("nesting_%d" % d, bytes(blk) + o + b"(e)" * 40 + c + b"(f)" * 60))
    # random mixes: no quotes, few, many
    for q in (0.0, 0.01, 0.1):
        out.append(("mix_quotes_%g" % q, _mix(rnd, B + 300, q)))
    if full:
        out.append(("long_nested", _nested(rnd, 9 * B + 17, maxdepth=40)))
        out.append(("long_mix", _mix(rnd, 12 * B + 5, 0.003)))
        out.append(("long_deep", b"".join(b"".join(_chain(rnd, rnd.choice((65, 96, 129, 200)))) for _ in range(80))))
        out.append(("long_quotes_only", b"'\"\"'" * 12000))
    for name, blk in out:
        assert 1024 <= len(blk) <= 65536, (name, len(blk))
    return out * 4 if full else out


DENSE = ("events_%d" % (B - 1), "events_%d" % B, "events_%d" % (B + 1), "node_across_batches", "nesting_65", "mix_quotes_0")


def engine_run(blocks, flags):
    import pyoracle as po
    import erlamsa_amd as ea
    data, off = po.pack(blocks)
    e = ea.Engine(0)
    e.configure(mutations=MUTS, patterns=PATS, max_case_bytes=4 << 20, big_case_bytes=32 << 20, flags=flags)
    e.upload_corpus(data, off)
    e.fuzz_batch(seed=SEED)
    got, st = e.download()
    dr, _ = e.diag()
    e.close()
    return got, st, dr


_ORACLE = {}


def oracle(full):
    """computed once per corpus and shared; never changed afterwards"""
    if full not in _ORACLE:
        import pyoracle as po
        import util
        data, off = po.pack([b for _, b in inputs(full)])
        _ORACLE[full] = util.oracle_live(data, off, seed=SEED, mutations=MUTS, patterns=PATS, max_case_bytes=64 << 20, chunk=1)
    return _ORACLE[full]


def run(full, verbose=True):
    """-> (cases, bad).  A case is bad unless the oracle's status is 0 and lanes on, lanes off and the oracle agree on everything."""
    ins = inputs(full)
    blocks = [b for _, b in ins]
    o = oracle(full)
    on = engine_run(blocks, 0)
    offr = engine_run(blocks, EH_FLAG_TREE_NO_LANES)
    bad = 0
    for i, (name, blk) in enumerate(ins):
        rows = [(int(o.status[i]), int(o.lens[i]), int(o.draws[i]), o.digests[i].tobytes())]
        for got, st, dr in (on, offr):
            rows.append((int(st[i]), len(got[i]), int(dr[i]), hashlib.sha1(got[i]).digest()))
        ok = rows[0][0] == 0 and rows[1] == rows[0] and rows[2] == rows[0]
        if verbose:
            print("%-26s %6d B  oracle/lanes/sequential: status %d/%d/%d len %d/%d/%d draws %d/%d/%d sha1 %s/%s/%s  %s" % (
                name, len(blk), rows[0][0], rows[1][0], rows[2][0], rows[0][1], rows[1][1], rows[2][1], rows[0][2], rows[1][2], rows[2][2],
                rows[0][3].hex()[:8], rows[1][3].hex()[:8], rows[2][3].hex()[:8], "ok" if ok else "BAD"))
        bad += 0 if ok else 1
    return len(ins), bad


def counters():
    """emulator build only: per block, (events committed by lane batches, lane batches, batches that fell short, parses, their events)"""
    import ctypes
    import erlamsa_amd.engine as eng
    ctr = (ctypes.c_ulonglong * 5).in_dll(eng.load_library(), "eh_emu_tree_lanes")
    res = {}
    for name, blk in inputs(False):
        if name in DENSE or name == "quotes_only":
            before = list(ctr)
            engine_run([blk], 0)
            res[name] = tuple(int(ctr[k]) - before[k] for k in range(5))
    return res


# ---- pytest ----------------------------------------------------------------------------------------------------------------
def _self(lib, mode):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=dict(os.environ, ERLAMSA_HIP_LIB=lib), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]
    return r.stdout


def test_emulated_lane_batches_agree_with_the_sequential_loop_and_the_oracle():
    import build_emu
    out = _self(build_emu.build(), "emu")
    assert "bad 0" in out, out[-6000:]


def test_emulated_lane_batches_are_committed_on_bracket_dense_blocks():
    """On the bracket-dense blocks every parse must commit nearly all of its events through lane batches (what is left is a tail
    shorter than 4 S events) and no batch may fall short; the block of quotes only must fall back: its batches stop at once.
    (Counted by the emulator build, csrc/eh_tree.h TL_COUNT; a case parses once per tree mutator it tries.)"""
    import build_emu
    out = _self(build_emu.build(), "counters")
    # lines: "<name> = committed batches short parses events"
    rows = dict((ln.split()[0], [int(x) for x in ln.split()[2:]]) for ln in out.splitlines() if ln.split()[1:2] == ["="])
    for name in DENSE:
        committed, batches, short, parses, events = rows[name]
        assert parses >= 1 and batches >= parses and short == 0 and committed > events - parses * 4 * S, (name, rows[name])
    committed, batches, short, parses, events = rows["quotes_only"]
    assert parses >= 1 and batches >= parses and short == batches and committed < events // 4, rows["quotes_only"]


@pytest.mark.gpu
def test_lane_batches_agree_with_the_sequential_loop_and_the_oracle_on_the_device():
    total, bad = run(full=True)
    assert total == len(inputs(True)) and bad == 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "emu"
    if mode == "counters":
        for name, v in counters().items():
            print("%s = %d %d %d %d %d" % ((name,) + v))
        sys.exit(0)
    total, bad = run(full=mode == "full")
    print("cases %d bad %d" % (total, bad))
    sys.exit(1 if bad else 0)
