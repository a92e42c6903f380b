"""CPU tests of the reassignment log's arithmetic (sylph_amd/csrc/reassign_edges_plan.h, the very header reassign_edges.hip includes,
compiled with g++ through tests/reassign_edges_plan_capi.cpp) against numpy: the work list of the count launch, the window and
not-self rule, the threshold, the compaction order (a lane-by-lane replay of the count kernel), the capacity and its one retry, the
final order and merge — and the stand-alone sanitizer run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from .helpers import build_path

HERE = os.path.dirname(os.path.abspath(__file__))
HDR = os.path.join(HERE, "..", "sylph_amd", "csrc", "reassign_edges_plan.h")
SRC = os.path.join(HERE, "reassign_edges_plan_capi.cpp")
u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
NONE = 2**32 - 1
EDGE = np.dtype([("winner", np.uint32), ("loser", np.uint32), ("count", np.uint32)])


@pytest.fixture(scope="module")
def L():
    out, stale = build_path("sylph_reassign_edges_plan", [SRC, HDR], ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, SRC])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    lib.ep_constants.argtypes = [vp]
    lib.ep_n_windows.restype = u32
    lib.ep_n_windows.argtypes = [u32, u32]
    lib.ep_work_losers.restype = u32
    lib.ep_work_losers.argtypes = [vp, u32, vp]
    lib.ep_n_work_items.restype = u64
    lib.ep_n_work_items.argtypes = [u32, u32, u32]
    lib.ep_work_item.argtypes = [u32, u32, u32, vp]
    lib.ep_counts_in_window.argtypes = [u32, u32, u32, u32]
    lib.ep_reported.argtypes = [u32, u32]
    lib.ep_edge_bound.restype = u64
    lib.ep_edge_bound.argtypes = [vp, u32, u32]
    lib.ep_first_capacity.restype = u64
    lib.ep_first_capacity.argtypes = [u64, u32]
    lib.ep_retry_capacity.restype = u64
    lib.ep_retry_capacity.argtypes = [u64, u64]
    lib.ep_sort_and_merge.restype = u64
    lib.ep_sort_and_merge.argtypes = [vp, u64]
    lib.ep_model_count.restype = u64
    lib.ep_model_count.argtypes = [vp, vp, u32, u32, u32, vp, u64]
    k = np.zeros(8, dtype=np.uint64)
    lib.ep_constants(k.ctypes.data)
    assert int(k[0]) == NONE and int(k[1]) == 256 and int(k[2]) == 4 and int(k[5]) == EDGE.itemsize == 12
    lib.WINDOW_MAX, lib.WINDOW_DEFAULT, lib.FIRST_MIN, lib.FIRST_PER_RANK = int(k[3]), int(k[4]), int(k[6]), int(k[7])
    return lib


def offsets(rng, n_passing, empty_every=3, hi=50):
    """kmer_off of n_passing lists, every `empty_every`-th one (from the second) empty"""
    lens = rng.integers(1, hi, size=n_passing)
    if empty_every:
        lens[1::empty_every] = 0
    off = np.zeros(n_passing + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return off


def test_window_default_is_the_largest_and_fits_the_lds(L):
    assert L.WINDOW_DEFAULT == L.WINDOW_MAX == 8192                       # 32 KB of counters: a workgroup may hold 64 KB


@pytest.mark.parametrize("W", [1, 5, 64, 8192])
def test_work_list(L, W):
    rng = np.random.default_rng(W)
    o = np.zeros(3, dtype=np.uint32)
    for n_passing in (0, 1, W - 1, W, W + 1, 3 * W + 5):
        off = offsets(rng, n_passing)
        losers = np.zeros(max(1, n_passing), dtype=np.uint32)
        n_losers = L.ep_work_losers(off.ctypes.data, n_passing, losers.ctypes.data)
        want_losers = np.nonzero(np.diff(off.astype(np.int64)) > 0)[0]
        assert losers[:n_losers].tolist() == want_losers.tolist()
        nw = -(-n_passing // W)
        assert L.ep_n_windows(n_passing, W) == nw and L.ep_n_work_items(n_losers, n_passing, W) == n_losers * nw
        items = np.arange(n_losers * nw) if n_losers * nw <= 4000 else np.unique(np.concatenate([np.arange(50), n_losers * nw - 1 - np.arange(50), rng.integers(0, n_losers * nw, size=300)]))
        seen = set()
        for b in items.tolist():
            L.ep_work_item(b, n_passing, W, o.ctypes.data)
            slot, base, length = (int(v) for v in o)
            assert slot == b // nw and base == (b % nw) * W and length == min(W, n_passing - base) and 1 <= length
            seen.add((slot, base))
        assert len(seen) == len(items)                                     # every (loser, window) once
        if n_losers * nw <= 4000:                                          # together the windows of a loser cover every rank once
            covered = np.zeros(n_passing, dtype=np.int64)
            for b in range(nw):
                L.ep_work_item(b, n_passing, W, o.ctypes.data)
                covered[int(o[1]):int(o[1]) + int(o[2])] += 1
            assert (covered == 1).all()
    assert L.ep_work_losers(np.zeros(4, dtype=np.uint64).ctypes.data, 3, np.zeros(3, dtype=np.uint32).ctypes.data) == 0   # all empty: no item


def test_window_and_not_self_rule(L):
    for base, length in ((0, 64), (64, 64), (128, 5), (8192, 8192), (2**32 - 2 - 10, 10)):
        for w in (0, base - 1, base, base + 1, base + length - 2, base + length - 1, base + length, base + length + 1, NONE):
            if not 0 <= w <= NONE:
                continue
            for loser in (0, base, base + length - 1, base + length, w):
                want = base <= w < base + length and w != loser
                assert bool(L.ep_counts_in_window(w, loser, base, length)) == want, (w, loser, base, length)
    assert not L.ep_counts_in_window(NONE, 3, 0, 8192)                    # no winner: in no window


def test_threshold(L):
    assert not L.ep_reported(10, 11) and L.ep_reported(11, 11) and L.ep_reported(12, 11)
    assert not L.ep_reported(0, 0) and L.ep_reported(1, 0)                # min_count 0 behaves as 1
    assert not L.ep_reported(0, 1) and L.ep_reported(1, 1) and L.ep_reported(NONE, NONE) and not L.ep_reported(NONE - 1, NONE)


def numpy_edges(winner, off, n_passing, min_count):
    """(loser, winner) -> count over the winner array, thresholded; as a sorted structured array"""
    loser = np.repeat(np.arange(n_passing, dtype=np.int64), np.diff(off.astype(np.int64)))
    w = winner.astype(np.int64)
    keep = (w != NONE) & (w != loser)
    key, cnt = np.unique(loser[keep] * 2**32 + w[keep], return_counts=True)
    sel = cnt >= max(1, min_count)
    out = np.zeros(int(sel.sum()), dtype=EDGE)
    out["loser"], out["winner"], out["count"] = key[sel] >> 32, key[sel] & NONE, cnt[sel]
    return out


@pytest.mark.parametrize("W", [1, 63, 64, 256, 300, 8192])
def test_count_model_compaction_and_retry(L, W):
    """The count launch replayed lane by lane with the plan's functions: every work item's reported entries at consecutive slots
    from its reservation in ascending winner order (so the whole list is already in (loser, winner) order when the items run in
    turn), a list that is too small reports how much it needs, and the retry with that capacity holds everything."""
    rng = np.random.default_rng(1000 + W)
    for n_passing in sorted({1, 2, max(2, W - 1), W, W + 1, 3 * W + 5} if W <= 300 else {2, 700}):
        off = offsets(rng, n_passing, hi=60 if W <= 300 else 3000)
        n_q = int(off[-1])
        loser = np.repeat(np.arange(n_passing), np.diff(off.astype(np.int64)))
        edge_ranks = np.array([0, W - 1, W, W + 1, n_passing - 1], dtype=np.int64) % n_passing       # winners at the window edges
        winner = np.where(rng.random(n_q) < 0.6, rng.choice(edge_ranks, size=n_q), rng.integers(0, n_passing, size=n_q))
        winner = np.where(rng.random(n_q) < 0.1, NONE, winner)
        winner = np.where(rng.random(n_q) < 0.1, loser, winner).astype(np.uint32)                    # self-winners count nothing
        for min_count in (0, 1, 3, 11):
            want = numpy_edges(winner, off, n_passing, min_count)
            bound = L.ep_edge_bound(off.ctypes.data, n_passing, min_count)
            lens = np.diff(off.astype(np.int64))
            assert bound == int(np.minimum(n_passing - 1, lens // max(1, min_count)).sum()) >= len(want)
            small = len(want) // 2
            edges = np.zeros(max(1, small), dtype=EDGE)
            cursor = L.ep_model_count(winner.ctypes.data, off.ctypes.data, n_passing, W, min_count, edges.ctypes.data, small)
            assert cursor == len(want)
            assert np.array_equal(edges[:small], want[:small])             # what fitted is the head of the ordered list
            again = L.ep_retry_capacity(cursor, small)
            assert again == (cursor if cursor > small else 0)
            edges = np.zeros(max(1, cursor), dtype=EDGE)
            assert L.ep_model_count(winner.ctypes.data, off.ctypes.data, n_passing, W, min_count, edges.ctypes.data, cursor) == cursor
            assert L.ep_retry_capacity(cursor, cursor) == 0 and np.array_equal(edges[:cursor], want)


def test_counts_of_exactly_ten_and_eleven(L):
    off = np.array([0, 30, 30, 60], dtype=np.uint64)
    winner = np.array([2] * 10 + [1] * 11 + [0] * 9 + [0] * 11 + [1] * 10 + [2] * 9, dtype=np.uint32)
    edges = np.zeros(8, dtype=EDGE)
    n = L.ep_model_count(winner.ctypes.data, off.ctypes.data, 3, 8192, 11, edges.ctypes.data, 8)
    assert [tuple(int(v) for v in e) for e in edges[:n]] == [(1, 0, 11), (0, 2, 11)]   # the two counts of 10 stay out


def test_retry_sizing(L):
    assert L.ep_retry_capacity(0, 0) == 0 and L.ep_retry_capacity(5, 5) == 0 and L.ep_retry_capacity(6, 5) == 6 and L.ep_retry_capacity(2**32 - 1, 10) == 2**32 - 1
    # first capacity: the bound where it is small, else a floor of 2^16 edges or 16 per passing genome — never n_passing^2
    assert L.ep_first_capacity(0, 1000) == 0 and L.ep_first_capacity(123, 1000) == 123
    assert L.ep_first_capacity(10**9, 1000) == L.FIRST_MIN == 2**16
    assert L.ep_first_capacity(10**12, 10**5) == L.FIRST_PER_RANK * 10**5 < (10**5)**2
    off = np.array([0, 100, 100, 121, 10**6], dtype=np.uint64)            # lists of 100, 0, 21 and 999,879 k-mers, 4 passing
    assert L.ep_edge_bound(off.ctypes.data, 4, 11) == 3 + 0 + 1 + 3 and L.ep_edge_bound(off.ctypes.data, 4, 0) == 3 + 0 + 3 + 3
    assert L.ep_edge_bound(off.ctypes.data, 1, 1) == 0                    # one passing genome: nobody to lose to


def test_order_and_merge_of_shuffled_partial_lists(L):
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 50, 3000):
        full = np.zeros(n, dtype=EDGE)
        full["loser"], full["winner"], full["count"] = rng.integers(0, 40, size=n), rng.integers(0, 40, size=n), rng.integers(1, 1000, size=n)
        shuffled = full[rng.permutation(n)].copy()                          # partial lists of the same pairs, in any order
        buf = np.concatenate([shuffled, np.zeros(1, dtype=EDGE)])
        m = L.ep_sort_and_merge(buf.ctypes.data, n)
        key = full["loser"].astype(np.int64) * 2**32 + full["winner"]
        uk, inv = np.unique(key, return_inverse=True)
        sums = np.bincount(inv, weights=full["count"], minlength=len(uk)).astype(np.int64)
        assert m == len(uk)
        assert (buf["loser"][:m].astype(np.int64) * 2**32 + buf["winner"][:m]).tolist() == uk.tolist()   # (loser, winner) ascending, each once
        assert buf["count"][:m].tolist() == sums.tolist()


def test_standalone_program_runs_clean_under_the_sanitizers():
    """tests/reassign_edges_sanitize_main.cpp + the model, built with AddressSanitizer and UBSan into a program of its own and run
    on the CPU: nothing is loaded into this interpreter."""
    srcs = [os.path.join(HERE, "reassign_edges_sanitize_main.cpp"), SRC]
    exe, stale = build_path("sylph_reassign_edges_sanitize", srcs + [HDR])
    if stale:
        tmp = exe + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                               "-Werror", "-o", tmp] + srcs)
        os.replace(tmp, exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "reassign edges sanitize run ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    assert " 0 retries" not in p.stdout and " 0 edges" not in p.stdout
