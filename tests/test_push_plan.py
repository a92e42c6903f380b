"""CPU tests of the host-batch chunk cutter (sylph_amd/csrc/push_plan.h, compiled with g++ through tests/push_plan_capi.cpp): the chunks
push_host_batch sends to the device tile the batch, never split a pair, stay within the base, record and staging limits unless one
record (pair) alone exceeds them, and name the bytes and the 2-bit phase of their bases."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("r0", "r1", "b0", "b1", "byte0", "byte1", "phase", "off_bytes", "staged_off_at", "fits")
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    src = os.path.join(HERE, "push_plan_capi.cpp")
    hdr = os.path.join(HERE, "..", "sylph_amd", "csrc", "push_plan.h")
    key = hashlib.sha256(open(src, "rb").read() + open(hdr, "rb").read()).hexdigest()[:16]      # two checkouts on one machine: two libraries
    out = os.path.join(tempfile.gettempdir(), f"sylph_push_plan_{os.getuid()}_{key}.so")
    if not os.path.exists(out):
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, src])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    u64p = C.POINTER(C.c_uint64)
    lib.pp_constants.argtypes = [u64p]
    lib.pp_limits.argtypes = [C.c_int, C.c_uint64, u64p]
    lib.pp_chunks.argtypes = [u64p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, u64p, C.c_uint64]
    lib.pp_chunks.restype = C.c_int64
    _lib = lib
    return lib


@pytest.fixture(scope="module")
def K():
    v = (C.c_uint64 * 4)()
    load().pp_constants(v)
    return dict(zip(("STAGE_BYTES", "STAGE_BASE_BYTES", "MAX_CHUNK_BASES", "LIMIT_SLACK"), (int(x) for x in v)))


def limits(pinned, push_chunk_bytes):
    v = (C.c_uint64 * 2)()
    load().pp_limits(int(pinned), push_chunk_bytes, v)
    return int(v[0]), int(v[1])


def offsets(lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, dtype=np.uint64))
    return off


def chunks(off, paired, bpb, max_bytes, max_recs):
    """the walk of push_host_batch -> dict of int64 arrays, one entry per chunk"""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1
    cap = n + 1
    out = np.zeros((cap, len(FIELDS)), np.uint64)
    u64p = C.POINTER(C.c_uint64)
    got = load().pp_chunks(off.ctypes.data_as(u64p), n, int(paired), bpb, max_bytes, max_recs, out.ctypes.data_as(u64p), cap)
    assert got >= 0, "a chunk made no progress, or more chunks than records"
    return {f: out[:got, i].astype(np.int64) for i, f in enumerate(FIELDS)}


def check(off, paired, bpb, pinned, push_chunk_bytes, K, max_recs=None):
    """Every property a walk must have.  max_recs: in place of chunk_limits' (crafted tables that are to reach it with few records).
    -> the chunks, with `forced` (a single record or pair beyond the limits)"""
    off = np.asarray(off, dtype=np.uint64)
    o = off.astype(np.int64)
    n = len(o) - 1
    max_bytes, lim_recs = limits(pinned, push_chunk_bytes)
    # chunk_limits, from its inputs: the option, the device-slot bound for page-locked input, the staging buffer's split for pageable input
    assert max_bytes == min(push_chunk_bytes, 1 << 31 if pinned else 24 << 20)
    assert lim_recs == (4 << 20 if pinned else (K["STAGE_BYTES"] - (24 << 20)) // 8 - 2)
    max_recs = lim_recs if max_recs is None else max_recs
    limit = min(max_bytes * bpb, 1 << 31) - 8                                # bases of a chunk that is not forced
    assert limit <= (1 << 31) - 8
    c = chunks(off, paired, bpb, max_bytes, max_recs)
    r0, r1, b0, b1 = c["r0"], c["r1"], c["b0"], c["b1"]
    unit = 2 if paired else 1
    # tiles [0, n) in order: no gap, no overlap, no empty chunk
    assert len(r0) >= 1 and r0[0] == 0 and r1[-1] == n and np.array_equal(r0[1:], r1[:-1]) and (r1 > r0).all()
    assert np.array_equal(b0, o[r0]) and np.array_equal(b1, o[r1])
    if paired:
        assert ((r1 - r0) % 2 == 0).all() and (r0 % 2 == 0).all()            # no pair split
    recs, bases = r1 - r0, b1 - b0
    within = (bases <= limit) & (recs <= max_recs)
    forced = ~within
    assert (recs[forced] == unit).all()                                      # only a single record (pair) may exceed ...
    assert (bases[forced] > limit).all()                                     # ... and only by its bases
    # as many records as stay within: the next record (pair) would not have
    more = r1 < n
    nxt = np.minimum(r1 + unit, n)
    assert ((o[nxt] - b0 > limit) | (recs + unit > max_recs) | forced)[more].all()
    # bytes and phase
    assert np.array_equal(c["byte0"], b0 // bpb) and np.array_equal(c["byte1"], -(-b1 // bpb)) and np.array_equal(c["phase"], b0 % bpb)
    assert (c["byte0"] * bpb <= b0).all() and (c["byte1"] * bpb >= b1).all() and (c["phase"] == b0 - c["byte0"] * bpb).all()
    # staging (what pageable input asks): bases padded to 8, then the (n + 1) * 8 offset bytes
    nb, no = c["byte1"] - c["byte0"], (recs + 1) * 8
    pad = (nb + 7) // 8 * 8
    assert np.array_equal(c["off_bytes"], no) and np.array_equal(c["staged_off_at"], pad)
    fits = c["fits"].astype(bool)
    assert np.array_equal(fits, nb + no + 8 <= K["STAGE_BYTES"])             # the predicate: 8 bytes kept for aligning the offsets
    assert (pad + no <= K["STAGE_BYTES"])[fits].all()                        # what it says fits, fits
    if not pinned and max_recs <= lim_recs:
        assert fits[within].all()                                            # every chunk within the limits goes through one staging buffer
    c["forced"] = forced
    return c


def ref_chunks(off, paired, limit, max_recs):
    """the rule, spelled in Python: [(r0, r1)]"""
    o = [int(x) for x in off]
    n, unit, r0, out = len(o) - 1, 2 if paired else 1, 0, []
    while r0 < n:
        hi = r0
        while hi < min(n, r0 + max_recs) and o[hi + 1] - o[r0] <= limit:
            hi += 1
        if paired:
            hi -= (hi - r0) & 1
        if hi == r0:
            hi = min(n, r0 + unit)
        out.append((r0, hi))
        r0 = hi
    return out


def test_constants(K):
    assert K == {"STAGE_BYTES": 32 << 20, "STAGE_BASE_BYTES": 24 << 20, "MAX_CHUNK_BASES": 1 << 31, "LIMIT_SLACK": 8}
    # a pageable chunk within the limits fits one staging buffer whatever its bytes: bases (a partial byte at either end), pad, offsets
    for bpb in (1, 4):
        max_bytes, max_recs = limits(False, 1 << 31)
        nb_max = (max_bytes * bpb - 8) // bpb + 2
        assert (nb_max + 7) // 8 * 8 + (max_recs + 1) * 8 + 8 <= K["STAGE_BYTES"]


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("bpb", [1, 4])
def test_random_tables_small_chunks(K, paired, bpb):
    """short reads and the odd long or empty one against push_chunk_bytes from 64 up: dozens to thousands of chunks, starts at every phase"""
    rng = np.random.default_rng(17 + 2 * bpb + paired)
    phases = set()
    for chunk_bytes in (64, 65, 100, 777, 4096, 100000):
        for pinned in (False, True):
            n = 2 * int(rng.integers(1, 1500))
            lens = rng.integers(0, 302, size=n)
            lens[rng.integers(0, n, size=n // 50 + 1)] = 0
            lens[rng.integers(0, n, size=n // 100 + 1)] = rng.integers(300, 30000, size=n // 100 + 1)
            off = offsets(lens)
            c = check(off, paired, bpb, pinned, chunk_bytes, K)
            limit = min(limits(pinned, chunk_bytes)[0] * bpb, 1 << 31) - 8
            assert list(zip(c["r0"].tolist(), c["r1"].tolist())) == ref_chunks(off, paired, limit, limits(pinned, chunk_bytes)[1])
            phases |= set(c["phase"].tolist())
    assert phases == set(range(bpb))


@pytest.mark.parametrize("paired", [False, True])
def test_default_limits_on_large_tables(K, paired):
    """the limits as push_host_batch has them by default (64 MiB chunks; pageable: the staging buffer) and at the 2^31 bound"""
    rng = np.random.default_rng(5 + paired)
    reads = offsets(rng.integers(100, 152, size=1_500_000))                 # ~190 Mbases of short reads
    for bpb in (1, 4):
        for pinned in (False, True):
            c = check(reads, paired, bpb, pinned, 64 << 20, K)
            limit = ((64 << 20) if pinned else (24 << 20)) * bpb - 8
            total = int(reads[-1])
            # greedy over records (pairs) of at most 151 (302) bases: every chunk but the last is filled to within one of them
            assert not c["forced"].any() and -(-total // limit) <= len(c["r0"]) <= -(-total // (limit - 302))
    # page-locked input with the option at its top: 2^31 - 8 bases per chunk, whatever the bytes
    contigs = offsets(rng.integers(1, 400_000_000, size=60))
    for bpb in (1, 4):
        c = check(contigs, paired, bpb, True, 1 << 31, K)
        assert (c["b1"] - c["b0"] <= (1 << 31) - 8).all() and len(c["r0"]) > 2
    # records that reach max_recs before the bytes: pageable 2^20 - 2, page-locked 2^22
    tiny = offsets(rng.integers(0, 4, size=2_300_000))
    c = check(tiny, paired, 1, False, 64 << 20, K)
    assert (c["r1"] - c["r0"]).tolist() == [(1 << 20) - 2, (1 << 20) - 2, 2_300_000 - 2 * ((1 << 20) - 2)]
    tiny = offsets(rng.integers(0, 2, size=(1 << 22) + 10))
    c = check(tiny, paired, 4, True, 64 << 20, K)
    assert (c["r1"] - c["r0"]).tolist() == [1 << 22, 10]


@pytest.mark.parametrize("bpb", [1, 4])
def test_record_longer_than_a_chunk(K, bpb):
    """forced progress: the long record (its pair) is a chunk of its own, first, in the middle and last; the predicate says whether it
    still goes through one staging buffer"""
    for paired in (False, True):
        unit = 2 if paired else 1
        seen = set()
        for long_bases in (25 << 20, 26 << 20, 40 << 20, 4 * (31 << 20), 4 * (33 << 20)):
            for where in ("first", "middle", "last"):
                short = [150] * 6
                lens = {"first": [long_bases, 100] + short, "middle": short + [100, long_bases] + short, "last": short + [long_bases, 100]}[where]
                off = offsets(lens)
                c = check(off, paired, bpb, False, 64 << 20, K)
                at = lens.index(long_bases) // unit * unit
                i = int(np.searchsorted(c["r1"], at, side="right"))           # the chunk that holds it
                limit = (24 << 20) * bpb - 8
                is_forced = long_bases + (100 if paired else 0) > limit
                assert bool(c["forced"][i]) == is_forced and c["forced"].sum() == int(is_forced)
                if is_forced:
                    assert c["r0"][i] == at and c["r1"][i] == at + unit
                    nb = int(c["byte1"][i] - c["byte0"][i])
                    assert bool(c["fits"][i]) == (nb + (unit + 1) * 8 + 8 <= K["STAGE_BYTES"])
                    seen.add(bool(c["fits"][i]))
        assert seen == {False, True}                                          # forced chunks of both kinds were among them
        # the same at the smallest chunk size, where most records are "long": one record (pair) per chunk, all of them through staging
        lens = [60, 56, 57, 300, 0, 49, 48, 8, 100, 3]
        c = check(offsets(lens), paired, bpb, False, 64, K)
        assert c["fits"].all()
        if bpb == 1:
            assert c["forced"].tolist() == ([True, True, False, False, True] if paired else [True, False, True, True, False, False, True, False])


def test_zero_length_records_at_a_boundary(K):
    # 64-byte chunks of ASCII: 56 bases.  Empty records behind a full chunk still belong to it (their offsets do not exceed the limit).
    c = check(offsets([56, 0, 0, 10]), False, 1, False, 64, K)
    assert list(zip(c["r0"].tolist(), c["r1"].tolist())) == [(0, 3), (3, 4)]
    c = check(offsets([56, 0, 0, 0, 10, 0]), True, 1, False, 64, K)
    assert list(zip(c["r0"].tolist(), c["r1"].tolist())) == [(0, 4), (4, 6)]
    c = check(offsets([56, 0, 0, 10, 0, 0]), True, 1, False, 64, K)           # the pair (0, 10) does not fit behind (56, 0): it starts the next
    assert list(zip(c["r0"].tolist(), c["r1"].tolist())) == [(0, 2), (2, 6)]
    c = check(offsets([0, 0, 57, 0, 0, 56, 0]), False, 1, False, 64, K)       # empties in front of a forced record: a chunk of their own
    assert list(zip(c["r0"].tolist(), c["r1"].tolist())) == [(0, 2), (2, 3), (3, 7)] and c["forced"].tolist() == [False, True, False]
    # packed: 64 bytes hold 256 bases, 248 per chunk; the chunk behind starts mid-byte
    c = check(offsets([247, 0, 1, 0, 3, 0]), False, 4, True, 64, K)
    assert list(zip(c["r0"].tolist(), c["r1"].tolist())) == [(0, 4), (4, 6)] and c["phase"].tolist() == [0, 0] and c["byte0"].tolist() == [0, 62]
    c = check(offsets([245, 0, 5, 0]), False, 4, True, 64, K)
    assert list(zip(c["r0"].tolist(), c["r1"].tolist())) == [(0, 2), (2, 4)] and c["phase"].tolist() == [0, 1] and c["byte0"].tolist() == [0, 61]


@pytest.mark.parametrize("paired", [False, True])
def test_all_records_empty_and_max_recs(K, paired):
    for n in (2, 10, 11 * 2):
        for max_recs in ([] if paired else [1]) + [2, 5, 7, 100]:        # (chunk_limits never goes below two records: a pair is one unit)
            c = check(np.zeros(n + 1, np.uint64), paired, 1, False, 64, K, max_recs=max_recs)
            step = max(2 if paired else 1, max_recs - (max_recs & 1 if paired else 0))
            assert (c["r1"] - c["r0"]).tolist() == [step] * (n // step) + ([n % step] if n % step else [])
            assert (c["b0"] == 0).all() and (c["b1"] == 0).all() and (c["byte1"] == 0).all() and c["fits"].all()
    # max_recs before the bytes, with bases in the records
    rng = np.random.default_rng(3)
    off = offsets(rng.integers(0, 9, size=400))
    for max_recs in (5, 6, 64):
        c = check(off, paired, 4, True, 4096, K, max_recs=max_recs)
        limit = 4096 * 4 - 8
        assert list(zip(c["r0"].tolist(), c["r1"].tolist())) == ref_chunks(off, paired, limit, max_recs)
        assert (c["r1"] - c["r0"]).max() == max_recs - (max_recs & 1 if paired else 0)
