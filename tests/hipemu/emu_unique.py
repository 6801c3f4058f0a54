#!/usr/bin/env python3
"""The uniqueness filter (erlamsa_amd/csrc/eh_unique.h: eh_result_digests, eh_result_unique, eh_result_download_select,
eh_selftest_unique) against values that come from Python alone: zlib.crc32, a table CRC-32C written here from its polynomial and
pinned by the check value, and a dict keyed by bytes for first occurrences.

  ERLAMSA_HIP_LIB=build/liberlamsa_hip_emu.so python tests/hipemu/emu_unique.py [cases of the end-to-end batches]

tests/test_emulated_unique.py runs it on the CPU wavefront emulator (64 cases), tests/test_gpu_unique.py calls the same functions on
the real library (4096 cases)."""
import os
import re
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import erlamsa_amd as ea
from erlamsa_amd import api, engine
from erlamsa_amd.engine import EngineError

P = engine.UNIQUE_PIECE_BYTES
HTTP = b"GET /index.html HTTP/1.1\r\nHost: fuzz.net\r\n\r\n"
BYTE_MUTATORS, BYTE_PATTERNS = "bd,bf,bi,bei,bed,ber,br", "od,nd,bu"

_T32C = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0x82F63B78 if _c & 1 else _c >> 1
    _T32C.append(_c)


def crc32c(data):
    c = 0xFFFFFFFF
    for b in data:
        c = _T32C[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


assert crc32c(b"123456789") == 0xE3069283 and zlib.crc32(b"123456789") == 0xCBF43926


def digest(data):
    return (crc32c(data) << 32 | zlib.crc32(data)) if data else 0


# The same CRC-32C for the megabytes a real batch puts out, where a byte per interpreter step is too slow: every case is cut into a
# head and 1024-byte chunks, numpy walks all chunks of all cases side by side, and a case's chunk CRCs are put together with
# crc(A ++ B) = crc(A) * x^(8 |B|) ^ crc(B) in GF(2)[x] mod the polynomial.  digests_of_planted_lengths holds it against the
# byte loop above, and - run with CRC-32's polynomial - against zlib.
def _table(poly):
    t = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ poly if c & 1 else c >> 1
        t.append(c)
    return t


def _mulmod(a, b, poly):
    """a(x) * b(x) mod p(x), reflected: bit 31 is x^0"""
    p, m = 0, 1 << 31
    while m:
        if a & m:
            p ^= b
        b = (b >> 1) ^ poly if b & 1 else b >> 1
        m >>= 1
    return p


def crc_all(cases, poly, chunk=1024):
    table = _table(poly)
    tab = np.array(table, dtype=np.uint32)
    body = np.frombuffer(b"".join(c[len(c) % chunk:] for c in cases), dtype=np.uint8).reshape(-1, chunk)
    cols = np.ascontiguousarray(body.T)
    st = np.full(len(body), 0xFFFFFFFF, dtype=np.uint32)
    for j in range(chunk):
        st = tab[(st ^ cols[j]) & 0xFF] ^ (st >> 8)
    st = (st ^ 0xFFFFFFFF).tolist()
    xl = 1 << 31
    for _ in range(chunk):
        xl = _mulmod(xl, 1 << 23, poly)                        # x^(8 * chunk)
    out, k = [], 0
    for c in cases:
        v = 0
        if len(c) % chunk:
            v = 0xFFFFFFFF
            for b in c[:len(c) % chunk]:
                v = table[(v ^ b) & 0xFF] ^ (v >> 8)
            v ^= 0xFFFFFFFF
        for _ in range(len(c) // chunk):
            v = _mulmod(v, xl, poly) ^ st[k]
            k += 1
        out.append(v)
    return out


def digests_of(cases):
    return [hi << 32 | zlib.crc32(c) for hi, c in zip(crc_all(cases, 0x82F63B78), cases)]


def first_occurrences(cases, status):
    """first_of as include/erlamsa_hip.h defines it: the first EH_CASE_OK case with the same bytes; a case with another status is its own"""
    seen, out = {}, []
    for i, (b, s) in enumerate(zip(cases, status)):
        out.append(seen.setdefault(b, i) if s == 0 else i)
    return out


def pack(cases):
    off = np.zeros(len(cases) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(c) for c in cases], dtype=np.uint64)
    return np.frombuffer(b"".join(cases) + b"\0", dtype=np.uint8), off


def code(f, *a, **k):
    try:
        f(*a, **k)
    except EngineError as e:
        return e.code
    return 0


def piece_size_is_the_headers():
    h = open(os.path.join(ROOT, "include", "erlamsa_hip.h")).read()
    assert int(re.search(r"#define EH_UNIQUE_PIECE_BYTES (\d+)", h).group(1)) == P


def digests_of_planted_lengths(eng):
    """a. every length at which the digest kernel takes another path, packed back to back so that most cases start at odd offsets"""
    rng = np.random.Generator(np.random.PCG64(11))
    lens = [0, 1, 15, 16, 17, 31, 63, 64, 65, 1023, 1024, 1025, P - 1, P, P + 1, 2 * P + 1, 64 * P + 5]
    cases = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in lens]
    cases += [b"\0" * 777, b"\xff" * (P + 3)]
    data, off = pack(cases)
    assert sum(int(o) % 16 != 0 for o in off[:-1]) > len(cases) // 2
    dig, _ = eng.selftest_unique(data, off, np.zeros(len(cases), dtype=np.int32), dedup=False)
    want = [digest(c) for c in cases]
    assert digests_of(cases) == want and crc_all(cases, 0xEDB88320) == [zlib.crc32(c) for c in cases]       # the chunked CRC is the byte loop's
    bad = [(len(c), hex(int(g)), hex(w)) for c, g, w in zip(cases, dig, want) if int(g) != w]
    assert not bad, bad
    return len(cases)


def colliding_pair():
    """A != B of equal length with equal digest.  Both CRCs are affine over GF(2) for a fixed length, so the digest deltas of
    single-bit flips add up under xor; 80 such 64-bit vectors are linearly dependent, and Gaussian elimination names a subset of
    flips whose deltas cancel."""
    rng = np.random.Generator(np.random.PCG64(12))
    base = rng.integers(0, 256, size=40, dtype=np.uint8).tobytes()
    d0 = digest(base)
    rows = []
    for k in range(80):
        m = bytearray(base); m[k // 8] ^= 1 << (k % 8)
        rows.append((digest(bytes(m)) ^ d0, 1 << k))            # (delta, which flips made it)
    pivots = {}
    for v, who in rows:
        while v:
            top = v.bit_length() - 1
            if top not in pivots:
                pivots[top] = (v, who)
                break
            pv, pw = pivots[top]
            v ^= pv; who ^= pw
        if v == 0:
            other = bytearray(base)
            for k in range(80):
                if who >> k & 1:
                    other[k // 8] ^= 1 << (k % 8)
            other = bytes(other)
            assert other != base and digest(other) == d0
            return base, other
    raise AssertionError("80 vectors of 64 bits must be dependent")


def dedup_of_planted_cases(eng):
    """b. duplicates near and far, near misses, empties, cases that did not end EH_CASE_OK, multi-piece cases, a constructed collision"""
    rng = np.random.Generator(np.random.PCG64(13))
    rnd = lambda n: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    x, y, big = rnd(300), rnd(4097), rnd(2 * P + 1)
    cases = [x, x, y]                                            # 1: an exact duplicate at distance 1
    cases += [x[:-1] + bytes([x[-1] ^ 1]), bytes([x[0] ^ 0x80]) + x[1:], x[:150], b"", b"", rnd(17)]   # other last byte, other first byte, a prefix
    status = [0] * len(cases)
    cases += [x, y, x]; status += [1, 2, 5]                       # not EH_CASE_OK: their own first, and nobody's
    cases += [big, rnd(40), big, big[:-1] + bytes([big[-1] ^ 0xFF])]; status += [0, 0, 0, 0]
    cases += [rnd(int(n)) for n in rng.integers(1, 200, size=70)]; status += [0] * 70
    cases += [y, b"", x]; status += [0, 0, 0]                      # duplicates more than 64 cases away; the third empty one
    a, b = colliding_pair()
    c0 = len(cases)
    cases += [a, b, a, b]; status += [0, 0, 0, 0]
    data, off = pack(cases)
    dig, first = eng.selftest_unique(data, off, np.asarray(status, dtype=np.int32))
    assert [int(d) for d in dig] == [digest(c) for c in cases]
    want = first_occurrences(cases, status)
    got = [int(f) for f in first]
    assert got[:c0] == want[:c0], [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert got[9] == 9 and got[10] == 10 and got[11] == 11 and want[c0 - 1] == 0 and want[c0 - 3] == 2
    # the collision: B shares A's length and digest but not its bytes - never a duplicate of A; the second B is B's duplicate or unique
    assert got[c0:c0 + 3] == [c0, c0 + 1, c0] and got[c0 + 3] in (c0 + 1, c0 + 3), got[c0:]
    return len(cases)


def check_batch(eng, label):
    """c. the last batch of `eng`: digests, first_of and the totals against the downloaded bytes, download_select against them too"""
    outs, status = eng.download()
    n = len(outs)
    assert [int(d) for d in eng.digests()] == digests_of(outs), label
    first, n_unique, unique_bytes = eng.unique()
    want = first_occurrences(outs, status)
    assert [int(f) for f in first] == want, label
    uniq = [i for i in range(n) if status[i] == 0 and want[i] == i]
    assert n_unique == len(uniq) and unique_bytes == sum(len(outs[i]) for i in uniq), label
    assert eng.download_select(uniq) == [outs[i] for i in uniq], label
    for idx in (uniq[::-1], (uniq[:5] + uniq[:5] + [n - 1, 0, n - 1])):
        assert eng.download_select(idx) == [outs[i] for i in idx], label
    assert eng.download_select([]) == []
    ok = int((np.asarray(status) == 0).sum())
    return ok, len(uniq)


def end_to_end(n):
    """c. two workloads that repeat themselves - one 44-byte HTTP request under the full default tables, one random 256-byte block
    under the byte mutators - with and without EH_FLAG_ORDERED_OUTPUT, then another batch on the same context.
    At 4096 cases and seed (1, 2, 3) the oracle counts 42 % and 14 % duplicates; the test wants 5 % there.  The CPU emulator runs 64
    cases, where repeats are rare for the plain reason that few cases have gone before (the block workload has 1 in 64): there the
    test wants one duplicate per workload, which still keeps a batch without duplicates from passing.  On the emulator the HTTP
    batches also run under a work budget (max_case_work): two of the 64 cases take half a minute of emulated fuse otherwise, and the
    budget makes them - and a dozen more - end EH_CASE_BUDGET, a status the filter has to leave alone."""
    assert len(HTTP) == 44
    full = n >= 4096
    block = np.random.Generator(np.random.PCG64(14)).integers(0, 256, size=256, dtype=np.uint8).tobytes()
    shares = []
    for flags in (0, engine.EH_FLAG_ORDERED_OUTPUT):
        eng = ea.Engine(0)
        for name, inp, conf in (("http", HTTP, {} if full else {"max_case_work": 65536}), ("block", block, {"mutations": BYTE_MUTATORS, "patterns": BYTE_PATTERNS})):
            eng.configure(flags=flags, **conf)
            data, off = pack([inp] * n)
            eng.upload_corpus(data, off)
            eng.fuzz_batch(seed=(1, 2, 3))
            ok, uniq = check_batch(eng, (name, flags))
            print("%s flags=%d: %d distinct of %d ok cases" % (name, flags, uniq, ok))
            assert ok - uniq >= (0.05 * ok if full else 1), (name, flags, ok, uniq)
            shares.append((name, flags, ok, uniq))
        # the next batch on the same context: its own values, not the cached ones
        eng.fuzz_batch(seed=(4, 5, 6), n=max(n // 2, 1))
        check_batch(eng, ("second batch", flags))
        eng.close()
    return shares


def api_option(n):
    """d. fuzzer(unique) = the order-preserving dedup of fuzzer(); fuzz_batch(unique, return_status) also returns first_of
    (the HTTP workload at 4096 cases; the block workload on the emulator, whose default-table batches take a minute each)"""
    if n >= 4096:
        inp, opts = HTTP, {"seed": (1, 2, 3), "input": HTTP, "n": n, "on_engine_limit": "skip"}
    else:
        inp = np.random.Generator(np.random.PCG64(14)).integers(0, 256, size=256, dtype=np.uint8).tobytes()
        opts = {"seed": (1, 2, 3), "input": inp, "n": n, "mutations": BYTE_MUTATORS, "patterns": BYTE_PATTERNS}
    plain = api.fuzzer(opts)
    assert len(set(plain)) < len(plain), "the workload has no duplicates: nothing is tested"
    assert api.fuzzer(dict(opts, unique=True)) == list(dict.fromkeys(plain))
    assert api.fuzzer(dict(opts, unique=True, skip=n // 4)) == list(dict.fromkeys(api.fuzzer(dict(opts, skip=n // 4))))
    outs, status = api.fuzz_batch([inp] * n, opts, return_status=True)
    uouts, ustatus, first = api.fuzz_batch([inp] * n, dict(opts, unique=True), return_status=True)
    assert uouts == outs and list(ustatus) == list(status) and [int(f) for f in first] == first_occurrences(outs, status)


def errors():
    """e. call order and arguments"""
    eng = ea.Engine(0)
    assert code(eng.digests) == -5 and code(eng.unique) == -5 and code(eng.download_select, [0]) == -5      # EH_E_STATE: no batch yet
    eng.configure(mutations="bd,bf", patterns="od")
    data, off = pack([b"some input bytes"] * 8)
    eng.upload_corpus(data, off)
    eng.fuzz_batch(seed=(1, 2, 3))
    outs, _ = eng.download()
    assert code(eng.download_select, [0, 8]) == -1                                                            # EH_E_INVALID: index out of range
    idx = np.arange(8, dtype=np.uint64)
    need = sum(map(len, outs))
    buf = np.zeros(need, dtype=np.uint8)
    off = np.zeros(9, dtype=np.uint64)
    rc = eng.lib.eh_result_download_select(eng.h, idx.ctypes.data, 8, buf.ctypes.data, need - 1, off.ctypes.data)
    assert rc == -1 and int(off[8]) == need                                                                   # cap too small: off says what is needed
    assert eng.download_select(idx) == outs
    # a context with coalesced requests pending belongs to the coalescer
    t = eng.submit(b"a request", (1, 2, 3))
    assert code(eng.digests) == -5 and code(eng.unique) == -5 and code(eng.download_select, [0]) == -5
    assert code(eng.selftest_unique, data, np.zeros(2, dtype=np.uint64), np.zeros(1, dtype=np.int32)) == -5
    eng.flush()
    assert eng.poll(t) is not None
    eng.close()


def run(n):
    piece_size_is_the_headers()
    eng = ea.Engine(0)
    nd = digests_of_planted_lengths(eng)
    nu = dedup_of_planted_cases(eng)
    eng.close()
    shares = end_to_end(n)
    api_option(n)
    errors()
    return nd, nu, shares


if __name__ == "__main__":
    nd, nu, shares = run(int(sys.argv[1]) if len(sys.argv) > 1 else 64)
    print("unique ok: %d digest cases, %d dedup cases, %s" % (nd, nu, shares))
