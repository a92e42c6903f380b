"""CPU tests of the filter dedup's plan (sylph_amd/csrc/a10_plan.h, the very header a10.hip includes, compiled with g++ through
tests/a10_plan_capi.cpp): hashes, keys and filter geometry against the numpy restatement (tests/helpers.py) and the oracle's Python
model; the class map of the partitioned pass for every B; the slot of a word inside its range, the slices and their escalation; the
grid; the walk's cut search; and a sequential model of the whole range pass, written from the header's functions alone, against
"not the first operation of its reduced-key class".  Plus the stand-alone sanitizer run of that model."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import pyref

from .helpers import a10_filter_geometry, a10_item_hash, a10_reduced_key, build_path
from .test_replay_plan import BucketMap

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "sylph_amd", "csrc")
HDRS = [os.path.join(CSRC, "a10_plan.h"), os.path.join(CSRC, "replay_plan.h")]
SRC = os.path.join(HERE, "a10_plan_capi.cpp")
NAMES = ("FX_K", "GOLD", "NO_OP", "MAX_FILTERS", "TILE_OCC", "OPS_BLK_PER_TILE", "RNG_SLOT_BITS", "RNG_CAND", "RNG_TAB", "RNG_WORDS", "MAX_SPLIT", "MAX_SLICES",
         "SLICE_STOP", "MAX_COARSE", "XCDS", "RNG_TPB", "RID_RANK_MAX", "RID_MARKER_BIT", "INVALID_HASH")
SPLITS = (1, 2, 4, 8)
FILTERS = [(1e-4, 10_000_000), (0.05, 2500), (0.3, 600), (1e-3, 5000)]       # (fpr, capacity) of tests/test_oracle.py's parametrisation


@pytest.fixture(scope="module")
def L():
    out, stale = build_path("sylph_a10_plan", [SRC] + HDRS, ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, SRC])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    for name, res, args in (
            ("ap_map_bytes", C.c_uint32, []), ("ap_constants", None, [u64p]), ("ap_item_hash", None, [u64p, u64p, C.c_uint64, u64p]),
            ("ap_filter_geometry", C.c_int, [C.c_uint64, C.c_double, C.c_int, u32p]), ("ap_reduced_key", None, [u64p, C.c_uint64, C.c_uint32, C.c_uint32, u64p]),
            ("ap_op_key", C.c_uint64, [C.c_uint64, C.c_uint32]), ("ap_op_word", C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32]),
            ("ap_table_geometry", None, [C.c_uint64, u64p]), ("ap_table_home", C.c_uint32, [C.c_uint64, C.c_uint32]),
            ("ap_fits", C.c_int, [C.c_uint64] * 4), ("ap_verdict_good", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint64]),
            ("ap_cut_tile", None, [u32p, C.c_uint32, C.c_uint64, u64p]), ("ap_class_map", None, [C.c_uint64, C.c_uint32, C.POINTER(BucketMap)]),
            ("ap_class_range", C.c_uint64, [C.c_uint32]), ("ap_class_of_keys", None, [C.POINTER(BucketMap), u32p, C.c_uint64, u32p]),
            ("ap_range_lo_keys", None, [C.c_uint32, u32p, C.c_uint64, u32p]), ("ap_range_geometry", None, [C.c_uint32, C.c_uint32, u32p]),
            ("ap_range_slots", None, [u32p, C.c_uint64, u32p, u32p, u32p]), ("ap_slice_of", None, [u32p, C.c_uint64, C.c_uint32, u32p]),
            ("ap_next_slices", C.c_uint32, [C.c_uint32, C.c_uint32]), ("ap_range_of_blocks", None, [C.c_uint32, C.c_uint32, u32p, u32p]),
            ("ap_range_grid", C.c_uint32, [C.c_uint32, C.c_uint32]), ("ap_table_homes", None, [u64p, C.c_uint64, u32p, u32p]),
            ("ap_partitioned_pass", C.c_int, [u64p, C.c_uint32, C.c_uint64, C.c_double, C.c_uint32, u8p, u32p, u32p])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    assert lib.ap_map_bytes() == C.sizeof(BucketMap)
    v = np.zeros(len(NAMES), np.uint64)
    lib.ap_constants(p(v))
    lib.K = {k: int(x) for k, x in zip(NAMES, v)}
    return lib


def p(a):
    return a.ctypes.data_as(C.POINTER({1: C.c_uint8, 4: C.c_uint32, 8: C.c_uint64}[a.dtype.itemsize]))


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def geometry(L, capacity, fpr, j=0):
    m = np.zeros(2, np.uint32)
    return L.ap_filter_geometry(capacity, fpr, j, p(m)), int(m[0]), int(m[1])


def reduced_keys(L, h, fp_mask, nb_mask):
    out = np.zeros(len(h), np.uint64)
    L.ap_reduced_key(p(h), len(h), fp_mask, nb_mask, p(out))
    return out


# ---- hashes and keys -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fpr,cap0", FILTERS)
def test_hashes_and_geometry_equal_the_numpy_restatement(L, fpr, cap0):
    rng = np.random.default_rng(cap0)
    n = 100_000
    km = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
    marker = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    h = np.zeros(n, np.uint64)
    L.ap_item_hash(p(km), p(marker), n, p(h))
    assert np.array_equal(h, a10_item_hash(km, marker))
    h[:64] &= np.uint64(0xFFFFFFFF)                                       # fingerprint 0 becomes 1
    for j in range(L.K["MAX_FILTERS"]):
        ok, fp_mask, nb_mask = geometry(L, cap0, fpr, j)
        fp_bits, nb = a10_filter_geometry(fpr * 0.9 ** j, cap0 << j)
        assert ok == (nb <= 1 << 31) and fp_mask == (1 << fp_bits) - 1 and nb_mask == (nb - 1) & 0xFFFFFFFF, (fpr, cap0, j)
        g = reduced_keys(L, h, fp_mask, nb_mask)
        assert np.array_equal(g, a10_reduced_key(h, fpr * 0.9 ** j, cap0 << j)) and int(g.max()) < 1 << 63 and int((g >> np.uint64(32)).min()) >= 1
    # the operation word: the upper half of the mixed class key above the operation id
    ok, fp_mask, nb_mask = geometry(L, cap0, fpr)
    g = a10_reduced_key(a10_item_hash(km[:300], marker[:300]), fpr, cap0)
    with np.errstate(over="ignore"):
        want = ((g * np.uint64(L.K["GOLD"])) & np.uint64(0xFFFFFFFF00000000)) | np.arange(300, dtype=np.uint64)
    assert [L.ap_op_word(fp_mask, nb_mask, int(km[i]), int(marker[i]), i) for i in range(300)] == want.tolist()


def test_geometry_refuses_more_than_2_31_buckets(L):
    assert geometry(L, (1 << 31) - 1, 1e-4, 2)[0] == 1 and geometry(L, (1 << 31) - 1, 1e-4, 3)[0] == 0      # 2^33 / 4 buckets; 2^34 / 4
    assert geometry(L, 10_000_000, 1e-4, 7)[0] == 1                      # the default filter's last growth step


def test_item_hash_equals_the_oracle_model(L):
    rng = np.random.default_rng(3)
    km = rng.integers(0, 1 << 62, size=300, dtype=np.uint64)
    marker = rng.integers(0, 1 << 64, size=300, dtype=np.uint64)
    h = np.zeros(300, np.uint64)
    L.ap_item_hash(p(km), p(marker), 300, p(h))
    assert L.K["FX_K"] == pyref._FX_K and L.K["GOLD"] == pyref._GOLD
    assert h.tolist() == [pyref._item_hash(int(k), (int(m) & 0xFFFFFFFF, int(m) >> 32)) for k, m in zip(km, marker)]


def test_op_key_orders_record_then_rank_then_marker(L):
    M, R = L.K["RID_MARKER_BIT"], L.K["RID_RANK_MAX"]
    assert R == (1 << 20) - 1

    def key(rec, rank, w, flags=M):
        return L.ap_op_key(flags | (rank << 42) | rec, w)
    order = [key(6, 0, 0), key(6, 0, 1), key(6, 1, 0), key(6, R, 0), key(6, R, 1), key(7, 0, 0), key(7, R, 1), key(8, 0, 0)]      # mate 1 (6) before mate 2 (7)
    assert order == sorted(order) and len(set(order)) == len(order)
    assert key(6, R, 1) == (6 << 21) | (R << 1) | 1 and key((1 << 42) - 1, R, 1) == (1 << 63) - 1
    assert key(6, 5, 1, flags=M | (1 << 62)) == key(6, 5, 1, flags=0)    # the marker and filter bits of the rid do not count


# ---- which pass, tables, cut -----------------------------------------------------------------------------------------------------
def test_fits_verdict_and_walk_tables(L):
    cap = 10_000_000
    assert L.ap_fits(100, cap // 2, 0, cap) and not L.ap_fits(100, cap // 2 + 1, 0, cap)
    assert not L.ap_fits(100, 50, 1, cap) and not L.ap_fits(1 << 31, 50, 0, cap) and L.ap_fits((1 << 31) - 1, 0, 0, cap)
    assert L.ap_verdict_good(0, cap, cap) and not L.ap_verdict_good(0, cap + 1, cap) and not L.ap_verdict_good(1, 5, cap)
    out = np.zeros(2, np.uint64)
    for remaining in (0, 1, 511, 512, 513, 10**6, 1 << 30):
        L.ap_table_geometry(remaining, p(out))
        slots, shift = int(out[0]), int(out[1])
        assert slots >= max(1024, 2 * remaining) and slots & (slots - 1) == 0 and (slots == 1024 or slots < 4 * remaining) and slots == 1 << (64 - shift)
        assert all(L.ap_table_home(g, shift) < slots for g in (0, 1, (1 << 63) - 1, (1 << 64) - 1, 0x123456789ABCDEF))


def test_cut_tile_against_a_prefix_sum(L):
    rng = np.random.default_rng(8)
    out = np.zeros(2, np.uint64)

    def cut(counts, cap):
        L.ap_cut_tile(p(counts), len(counts), cap, p(out))
        return int(out[0]), int(out[1])
    for n_tiles in (1, 2, 37, 1000):
        counts = rng.integers(0, 2049, size=n_tiles).astype(np.uint32)
        counts[rng.integers(0, n_tiles, size=n_tiles // 4)] = 0
        before = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
        total = int(before[-1])
        caps = {0, 1, total // 2, max(0, total - 1)} | {int(v) for v in before[:-1]} | {int(v) - 1 for v in before[1:] if v > 0}    # a tile's first and last operation
        for cap in sorted(caps):
            if cap >= total:
                continue
            tile = int(np.searchsorted(before, cap, side="right")) - 1   # inserting operation number cap (0-based) lies in this tile
            assert cut(counts, cap) == (tile, int(before[tile])) and before[tile] <= cap < before[tile + 1], (n_tiles, cap)
        for cap in (total, total + 1, 1 << 40):                            # no tile reaches the capacity
            assert cut(counts, cap) == (n_tiles, total)
    assert cut(np.zeros(0, np.uint32), 0) == (0, 0)


# ---- the class map ---------------------------------------------------------------------------------------------------------------
def class_map(L, n_expect, range_words=None):
    bm = BucketMap()
    L.ap_class_map(n_expect, L.K["RNG_WORDS"] if range_words is None else range_words, C.byref(bm))
    return bm


def class_of(L, bm, keys):
    keys = u32(keys)
    out = np.zeros(len(keys), np.uint32)
    L.ap_class_of_keys(C.byref(bm), p(keys), len(keys), p(out))
    return out.astype(np.int64)


def lo_keys(L, B, c):
    c = u32(c)
    out = np.zeros(len(c), np.uint32)
    L.ap_range_lo_keys(B, p(c), len(c), p(out))
    return out.astype(np.int64)


def test_class_map_and_its_inverse_for_every_B(L):
    W, MAXC = L.K["RNG_WORDS"], L.K["MAX_COARSE"]
    assert MAXC == 4096
    checked = 0
    for B in range(1, MAXC + 1):
        bm = class_map(L, B * W // 2)                                     # 2 n / W = B
        rng_w = (2**32 + B - 1) // B + 1
        assert (bm.B, bm.sh, bm.mult, bm.composite) == (B, 32, B, 1) and L.ap_class_range(B) == rng_w and bm.range_hs == min(rng_w, 0xFFFFFFFF), B
        c = np.arange(B, dtype=np.int64)
        lo = lo_keys(L, B, c)
        hi = np.concatenate([lo[1:] - 1, [2**32 - 1]])                    # the highest key of a range: the one before the next range's lowest
        assert lo[0] == 0 and (np.diff(lo) > 0).all(), B
        # the lowest and highest key of every range map to it, their outer neighbours to the neighbouring ranges
        assert np.array_equal(class_of(L, bm, lo), c) and np.array_equal(class_of(L, bm, hi), c), B
        assert np.array_equal(class_of(L, bm, lo[1:] - 1), c[:-1]) and np.array_equal(class_of(L, bm, hi[:-1] + 1), c[1:]), B
        # so bucket_of_key(key) == c implies lo <= key, and key - lo < range: the subtraction in the range kernel never wraps
        assert (hi - lo).min() >= 0 and (hi - lo).max() < rng_w, B
        checked += B
    assert checked == MAXC * (MAXC + 1) // 2
    # the clamps: one range for the smallest samples (width 2^32 + 1, the 32-bit field saturated), MAX_COARSE for the largest
    for n in (0, 1, W // 2 - 1, W - 1):
        bm = class_map(L, n)
        assert bm.B == 1 and bm.range_hs == 0xFFFFFFFF and L.ap_class_range(1) == 2**32 + 1
    assert class_map(L, W).B == 2 and class_map(L, MAXC * W // 2).B == MAXC and class_map(L, 10**12).B == MAXC and class_map(L, 2**40).B == MAXC
    assert class_map(L, 1000, 512).B == 3


# ---- slots, slices -----------------------------------------------------------------------------------------------------------------
def range_geometry(L, B, split):
    g = np.zeros(3, np.uint32)
    L.ap_range_geometry(B, split, p(g))
    return g


def slots_of(L, res, geo):
    res = u32(res)
    part, local = np.zeros(len(res), np.uint32), np.zeros(len(res), np.uint32)
    L.ap_range_slots(p(res), len(res), p(geo), p(part), p(local))
    return part.astype(np.int64), local.astype(np.int64)


def reachable_slice_counts(L):
    """Every slice count the escalation can produce from 1, by n_over (the first step is ceil(n_over / 256), capped: every P in 3..4096 — a
    range may hold hundreds of thousands of words), and the longest chain."""
    seen, longest, M = {1}, 0, L.K["MAX_SLICES"]
    for P in range(3, M + 1):                                              # the lowest and highest n_over of every first step
        assert L.ap_next_slices(1, 256 * P - 255) == P == L.ap_next_slices(1, 256 * P), P
    assert L.ap_next_slices(1, 513) == 3 and all(L.ap_next_slices(1, n) == M for n in (256 * M + 1, 10**7, 2**31, 2**32 - 1))
    for P in range(3, M + 1):
        steps = 0                                                           # escalations behind the first slice count
        while True:
            assert 1 < P <= L.K["MAX_SLICES"]
            seen.add(P)
            nxt = L.ap_next_slices(P, 513)
            assert nxt == 0 or nxt > P                                      # it never restarts with the same slices
            assert (nxt == 0) == (P >= L.K["SLICE_STOP"])                   # the stop rule, stated once
            if not nxt:
                break
            P, steps = nxt, steps + 1
        longest = max(longest, steps)
    return seen, longest


def test_range_slots_and_slices(L):
    S = 1 << L.K["RNG_SLOT_BITS"]
    assert S == 1 << 17 and L.K["MAX_SPLIT"] == 8
    rng = np.random.default_rng(4)
    for split in SPLITS:
        for B in (1, 2, 3, 7, 1000, 4095, 4096, 65536):                  # (the last: ranges narrower than the slot space, were B allowed that far)
            geo = range_geometry(L, B, split)
            width = (2**32 + B - 1) // B + 1
            assert geo[0] == split and geo[1] == split * S and (geo[2] == 0) == (width <= split * S), (split, B)
            top = min(width, 2**32) - 1
            res = np.unique(np.concatenate([np.arange(0, min(top + 1, 70000)), np.linspace(0, top, 50001).astype(np.int64), top - np.arange(0, min(top + 1, 70000)),
                                            rng.integers(0, top + 1, size=50000)]))
            part, local = slots_of(L, res, geo)
            slot = part * S + local
            assert part.min() >= 0 and part.max() < split and local.min() >= 0 and local.max() < S, (split, B)
            assert (np.diff(slot) >= 0).all(), (split, B)                  # monotone in the residue; equal residues (equal upper halves): one slot
            if geo[2]:                                                      # a range wider than the slot space uses all of it, evenly
                # (slot_mult is rounded down, the product again: less than 2 below the exact quotient)
                assert slot[0] == 0 and slot[-1] >= split * S - 2 and (res * (split * S) / width - slot).max() < 2.0 and (slot <= res * (split * S) / width).all(), (split, B)
            else:
                assert np.array_equal(slot, res), (split, B)
    counts, longest = reachable_slice_counts(L)
    assert longest <= 3 and max(counts) == L.K["MAX_SLICES"] and L.ap_next_slices(1, 513) == 3 and L.ap_next_slices(1, 2**32 - 1) == L.K["MAX_SLICES"]
    local = np.arange(S, dtype=np.uint32)
    out = np.zeros(S, np.uint32)
    for P in sorted(counts):                                                # every local slot falls into exactly one slice below P; the slices are even
        L.ap_slice_of(p(local), S, P, p(out))
        assert (np.diff(out.astype(np.int64)) >= 0).all() and out[0] == 0 and out[-1] == P - 1, P
        n = np.bincount(out, minlength=P)
        assert len(n) == P and n.min() >= S // P and n.max() <= S // P + 1, P


def test_lds_table_homes_stay_inside_the_tables(L):
    rng = np.random.default_rng(6)
    v = np.concatenate([rng.integers(0, 1 << 63, size=100000, dtype=np.uint64), np.array([0, 1, (1 << 32) - 2, (1 << 63) - 1], np.uint64)])
    up, cls = np.zeros(len(v), np.uint32), np.zeros(len(v), np.uint32)
    L.ap_table_homes(p(v), len(v), p(up), p(cls))
    T = L.K["RNG_TAB"]
    assert up.max() < T and cls.max() < T and len(np.unique(up)) == T and len(np.unique(cls)) == T
    assert L.K["RNG_CAND"] * 2 <= T and L.K["RNG_CAND"] % L.K["RNG_TPB"] == 0 and T * 16 <= (1 << L.K["RNG_SLOT_BITS"]) // 8


# ---- the grid ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 7, 8, 9, 4095, 4096])
def test_grid_names_every_range_part_once(L, B):
    for split in SPLITS:
        n = L.ap_range_grid(B, split)
        assert n == -(-B // 8) * 8 * split
        c, part = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        L.ap_range_of_blocks(n, split, p(c), p(part))
        c, part = c.astype(np.int64), part.astype(np.int64)
        real = c < B
        assert part.max() < split and real.sum() == B * split and len(set(zip(c[real].tolist(), part[real].tolist()))) == B * split, (B, split)
        assert (c[~real] >= B).all() and (~real).sum() == n - B * split                                # padding blocks
        for cc in (0, B // 2, B - 1):                                       # the workgroups of a range: 8 apart, parts in order
            blocks = np.flatnonzero(c == cc)
            assert np.array_equal(part[blocks], np.arange(split)) and (np.diff(blocks) == 8).all(), (B, split, cc)


# ---- the sequential model of the range pass ------------------------------------------------------------------------------------------
def sample(rng, n, copies=0):
    """n occurrence records {hash, rid, m0, m1}, two per record, a fifth of them repeats of others; then `copies` copies of one."""
    km = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
    m = rng.integers(0, 1 << 64, size=(n, 2), dtype=np.uint64)
    at, rep = rng.integers(0, n, size=n // 5), rng.integers(0, n, size=n // 5)
    km[at], m[at] = km[rep], m[rep]
    if copies:
        at = rng.choice(n, size=copies, replace=False)
        km[at], m[at] = km[at[0]], m[at[0]]
    i = np.arange(n, dtype=np.uint64)
    rid = np.uint64(1 << 63) | ((np.uint64(1) - (i & np.uint64(1))) << np.uint64(42)) | (i >> np.uint64(1))        # the record's second seed comes first in the arrays
    return np.ascontiguousarray(np.stack([km, rid, m[:, 0], m[:, 1]], axis=1))


def model_pass(L, recs, capacity, fpr, split):
    n = len(recs)
    marked, tail, stats = np.zeros(2 * n, np.uint8), np.zeros(2, np.uint32), np.zeros(3, np.uint32)
    assert L.ap_partitioned_pass(p(recs), n, capacity, fpr, split, p(marked), p(tail), p(stats)) == 0
    return marked.astype(bool), tail.tolist(), dict(B=int(stats[0]), max_P=int(stats[1]), workgroups=int(stats[2]))


def contained_by_classes(L, recs, capacity, fpr):
    """not the first operation of its reduced-key class by op_key — numpy, from the restated hashes"""
    km, rid, m = recs[:, 0], recs[:, 1], recs[:, 2:4]
    g = a10_reduced_key(a10_item_hash(np.repeat(km, 2), m.reshape(-1)), fpr, capacity)
    key = np.array([L.ap_op_key(int(r), w) for r in rid for w in (0, 1)], dtype=np.uint64)
    order = np.lexsort((key, g))
    first = np.ones(len(g), dtype=bool)
    first[1:] = g[order][1:] != g[order][:-1]
    contained = np.ones(len(g), dtype=bool)
    contained[order[first]] = False
    return contained


@pytest.mark.parametrize("fpr", [1e-4, 0.3])
@pytest.mark.parametrize("split", [1, 2, 4])
def test_range_pass_model_marks_all_but_the_first_of_every_class(L, fpr, split):
    rng = np.random.default_rng(int(fpr * 10**4) + split)
    capacity = 100_000                                                      # (at fpr 0.3: 2^20 classes — items of different k-mers meet)
    recs = sample(rng, 30_000)                                              # 60,000 operations: 7 ranges
    marked, tail, st = model_pass(L, recs, capacity, fpr, split)
    want = contained_by_classes(L, recs, capacity, fpr)
    assert st["B"] == 7 and st["workgroups"] == 7 * split and tail == [0, 2 * len(recs)] and L.ap_verdict_good(tail[0], tail[1], capacity)
    assert np.array_equal(marked, want) and want.sum() > 5000, np.flatnonzero(marked != want)[:10]
    if fpr == 0.3:
        exact = contained_by_classes(L, recs, 1 << 40, 1e-9)               # (31 fingerprint bits, 2^38 buckets: no item meets another)
        assert (want & ~exact).sum() > 100                                  # the filter's false positives are among the marks
    # 400 copies of one occurrence among 8,000 ordinary ones in ONE range: more second arrivals than the lists take — slices, good verdict
    recs = sample(rng, 8000, copies=400)
    marked, tail, st = model_pass(L, recs, capacity, fpr, split)
    want = contained_by_classes(L, recs, capacity, fpr)
    assert st["B"] == 1 and 1 < st["max_P"] <= L.K["MAX_SLICES"] and tail == [0, 16000], (st, tail)
    assert np.array_equal(marked, want) and want.sum() >= 2 * 399, np.flatnonzero(marked != want)[:10]
    # 3,000 copies: no slice is narrow enough — the verdict word is bumped (and the marks are not looked at: the walk takes the sample)
    recs = sample(rng, 8000, copies=3000)
    marked, tail, st = model_pass(L, recs, capacity, fpr, split)
    assert tail[0] >= 1 and tail[1] == 16000 and not L.ap_verdict_good(tail[0], tail[1], capacity) and st["max_P"] >= L.K["SLICE_STOP"], (st, tail)
    assert not (marked & ~contained_by_classes(L, recs, capacity, fpr)).any()       # what it did mark is no first of a class


def test_standalone_program_runs_clean_under_the_sanitizers():
    """tests/a10_plan_sanitize_main.cpp + the model, built with AddressSanitizer and UBSan into a program of its own and run on the CPU:
    nothing is loaded into this interpreter."""
    srcs = [os.path.join(HERE, "a10_plan_sanitize_main.cpp"), SRC]
    exe, stale = build_path("sylph_a10_plan_sanitize", srcs + HDRS)
    if stale:
        tmp = exe + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                               "-Werror", "-o", tmp] + srcs)
        os.replace(tmp, exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "a10 plan sanitize run ok: 18 samples" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
