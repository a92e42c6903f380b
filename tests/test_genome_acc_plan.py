"""CPU tests of the genome accumulator's plan (sylph_amd/csrc/genome_acc_plan.h, the very header genome_acc.hip and the host's
GenomeBatch include, compiled with g++ through tests/genome_acc_plan_capi.cpp): the cut of a file's contigs into pushes — every run
below the limit, contigs whole and in order, greedy, the first misfit at the right index — on random and crafted length lists, the
capacity rule, and the bounds at 2^32 - 2, 2^32 - 1 and 2^32.  Plus the stand-alone sanitizer run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from .helpers import build_path

HERE = os.path.dirname(os.path.abspath(__file__))
HDR = os.path.join(HERE, "..", "sylph_amd", "csrc", "genome_acc_plan.h")
SRC = os.path.join(HERE, "genome_acc_plan_capi.cpp")
LIMIT = 2**32 - 4096
TOP = 2**64 - 1


@pytest.fixture(scope="module")
def L():
    out, stale = build_path("sylph_genome_acc_plan", [SRC, HDR], ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, SRC])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    u64, ptr = C.c_uint64, C.c_void_p
    for name, res, args in (("gap_constants", None, [ptr]), ("gap_next_run", None, [ptr, u64, u64, u64, ptr]),
                            ("gap_cut", u64, [ptr, u64, u64, u64, ptr, u64, ptr]),
                            ("gap_capacity_for", u64, [u64, u64, u64]), ("gap_capacity_default", u64, [u64, u64]),
                            ("gap_contigs_fit", C.c_int, [u64, u64]), ("gap_seeds_fit", C.c_int, [u64, u64]), ("gap_push_fits", C.c_int, [u64, u64])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    k = (u64 * 4)()
    lib.gap_constants(k)
    lib.K = dict(zip("PUSH_LIMIT MAX_CONTIGS MAX_SEEDS FIRST_CAPACITY".split(), [int(v) for v in k]))
    return lib


def cut(L, lens, limit, start=0):
    """-> (runs [(first, n, bases)], index of the first misfit or len(lens))"""
    a = np.asarray(lens, dtype=np.uint64)
    runs = np.zeros(3 * (len(a) + 1), dtype=np.uint64)
    n_runs = C.c_uint64(0)
    at = L.gap_cut(a.ctypes.data if len(a) else None, len(a), start, limit, runs.ctypes.data, len(a) + 1, C.byref(n_runs))
    assert n_runs.value <= len(a)
    return [tuple(int(v) for v in runs[3 * r:3 * r + 3]) for r in range(n_runs.value)], int(at)


def check_cut(L, lens, limit, start=0):
    lens = [int(v) for v in lens]
    runs, at = cut(L, lens, limit, start)
    misfit = next((i for i in range(min(start, len(lens)), len(lens)) if lens[i] >= limit), len(lens))
    assert at == misfit                                              # the first misfit, at the right index
    nxt = min(start, len(lens))
    for first, n, bases in runs:
        assert first == nxt and n >= 1                               # whole contigs, in order, none left out
        assert bases == sum(lens[first:first + n]) and bases < limit   # every run below the limit
        nxt = first + n
        if nxt < misfit:
            assert bases + lens[nxt] >= limit                        # greedy: the next contig would not have fitted
    assert nxt == misfit
    return runs, at


def test_constants(L):
    assert L.K == dict(PUSH_LIMIT=LIMIT, MAX_CONTIGS=2**32 - 1, MAX_SEEDS=2**32 - 2, FIRST_CAPACITY=1 << 20)


def test_cut_on_crafted_lists(L):
    assert check_cut(L, [], LIMIT) == ([], 0)
    assert check_cut(L, [0], LIMIT) == ([(0, 1, 0)], 1)
    assert check_cut(L, [1], LIMIT) == ([(0, 1, 1)], 1)
    assert check_cut(L, [LIMIT - 1], LIMIT) == ([(0, 1, LIMIT - 1)], 1)
    assert check_cut(L, [LIMIT], LIMIT) == ([], 0)                                  # a contig of L bases alone is a misfit
    assert check_cut(L, [LIMIT - 1, 0, 1], LIMIT) == ([(0, 2, LIMIT - 1), (2, 1, 1)], 3)   # an empty contig always fits
    assert check_cut(L, [LIMIT - 2, 1, 1], LIMIT) == ([(0, 2, LIMIT - 1), (2, 1, 1)], 3)
    assert check_cut(L, [1, LIMIT - 2, 1], LIMIT) == ([(0, 2, LIMIT - 1), (2, 1, 1)], 3)
    assert check_cut(L, [5, 7, LIMIT, 5], LIMIT) == ([(0, 2, 12)], 2)               # the runs in front of the misfit are still cut
    assert check_cut(L, [5, 7, LIMIT, 5], LIMIT, start=3) == ([(3, 1, 5)], 4)       # ... and the caller may go on behind it
    assert check_cut(L, [5, 7, LIMIT, 5], LIMIT, start=2) == ([], 2)
    assert check_cut(L, [5], LIMIT, start=9) == ([], 1)
    assert check_cut(L, [TOP], LIMIT) == ([], 0)
    assert check_cut(L, [1, TOP, 1], LIMIT) == ([(0, 1, 1)], 1)
    assert check_cut(L, [0, 0, 0], 1) == ([(0, 3, 0)], 3)
    assert check_cut(L, [0, 1], 1) == ([(0, 1, 0)], 1)
    assert check_cut(L, [3, 3], 0) == ([], 0)                                       # no contig is below a limit of 0


def test_cut_with_sums_beyond_2_33(L):
    lens = [LIMIT - 1] * 9                                                          # 9 contigs, ~2^35.2 bases
    assert sum(lens) > 2**33
    runs, at = check_cut(L, lens, LIMIT)
    assert at == 9 and runs == [(i, 1, LIMIT - 1) for i in range(9)]
    lens = [2**31] * 5 + [2**31 - 4097, 1, 2**31]
    assert sum(lens) > 2**33
    runs, at = check_cut(L, lens, LIMIT)
    assert runs == [(0, 1, 2**31), (1, 1, 2**31), (2, 1, 2**31), (3, 1, 2**31), (4, 2, 2**32 - 4097), (6, 2, 2**31 + 1)]
    # five thousand contigs of a 5 Gbp genome at two limits: the number of pushes is what the sizes say
    rng = np.random.default_rng(5)
    lens = rng.integers(500_000, 1_500_000, size=5000)
    for limit in (LIMIT, 1 << 30):
        runs, at = check_cut(L, lens, limit)
        assert at == 5000 and int(lens.sum()) // limit + 1 <= len(runs) <= int(lens.sum()) // (limit - 1_500_000) + 1


@pytest.mark.parametrize("seed", range(8))
def test_cut_on_random_lists(L, seed):
    rng = np.random.default_rng(seed)
    for _ in range(150):
        limit = int(rng.integers(1, 5000))
        n = int(rng.integers(0, 60))
        lens = rng.integers(0, limit + limit // 8 + 1, size=n)
        lens[rng.random(n) < 0.1] = 0
        check_cut(L, lens, limit)
        # misfits skipped one by one (one genome per record): every other contig lands in exactly one run
        seen, at = [], 0
        while at < n:
            runs, at = check_cut(L, lens, limit, start=at)
            seen += [i for first, cnt, _ in runs for i in range(first, first + cnt)]
            at += 1
        assert seen == [i for i in range(n) if lens[i] < limit]


def test_next_run(L):
    a = np.array([4, 4, 9, 1], dtype=np.uint64)
    out = (C.c_uint64 * 3)()
    L.gap_next_run(a.ctypes.data, 4, 0, 9, out)
    assert list(out) == [0, 2, 8]
    L.gap_next_run(a.ctypes.data, 4, 2, 9, out)
    assert list(out) == [2, 0, 0]                                     # contig 2 alone holds the limit
    L.gap_next_run(a.ctypes.data, 4, 7, 9, out)
    assert list(out) == [4, 0, 0]                                     # behind the end: the empty run at n_contigs


def test_capacity_rule_is_monotone_and_reaches_need(L):
    S = L.K["MAX_SEEDS"]
    for first in (1, 64, 1000, L.K["FIRST_CAPACITY"]):
        cap, needs = 0, [0, 1, 63, 64, 65, 200, 2**20, 2**20 + 1, 2**31 + 1, S - 1, S]
        for need in needs:
            new = L.gap_capacity_for(cap, need, first)
            assert new >= need and new >= cap and new <= S
            assert new == cap or (new >= first and cap < need)                      # it only moves when it has to, never below the first size
            if cap and new != cap and new != S:
                assert new % cap == 0 and (new // cap) & (new // cap - 1) == 0      # by doubling
            assert L.gap_capacity_for(new, need, first) == new                      # a fixed point
            cap = new
        assert cap == S
    assert L.gap_capacity_for(0, 1, 64) == 64 and L.gap_capacity_for(64, 65, 64) == 128 and L.gap_capacity_for(64, 300, 64) == 512
    assert L.gap_capacity_for(0, 0, 64) == 0 and L.gap_capacity_for(0, 1, 0) == 1
    assert L.gap_capacity_default(0, 5) == 1 << 20 and L.gap_capacity_default(1 << 20, (1 << 20) + 1) == 1 << 21
    # monotone in need
    rng = np.random.default_rng(1)
    for _ in range(300):
        cap = int(rng.integers(0, 2**20))
        a, b = sorted(int(v) for v in rng.integers(0, 2**32 - 1, size=2))
        assert L.gap_capacity_for(cap, a, 64) <= L.gap_capacity_for(cap, b, 64)


def test_bounds_hold_exactly(L):
    # seeds: at most 2^32 - 2 (u32 indexes and a scan sentinel)
    assert L.gap_seeds_fit(0, 2**32 - 2) == 1 and L.gap_seeds_fit(0, 2**32 - 1) == 0 and L.gap_seeds_fit(0, 2**32) == 0
    assert L.gap_seeds_fit(2**32 - 3, 1) == 1 and L.gap_seeds_fit(2**32 - 2, 0) == 1 and L.gap_seeds_fit(2**32 - 2, 1) == 0
    assert L.gap_seeds_fit(2**32 - 1, 0) == 0 and L.gap_seeds_fit(TOP, TOP) == 0 and L.gap_seeds_fit(1, TOP) == 0
    # contigs: below 2^32
    assert L.gap_contigs_fit(0, 2**32 - 2) == 1 and L.gap_contigs_fit(0, 2**32 - 1) == 1 and L.gap_contigs_fit(0, 2**32) == 0
    assert L.gap_contigs_fit(2**32 - 2, 1) == 1 and L.gap_contigs_fit(2**32 - 1, 1) == 0 and L.gap_contigs_fit(TOP, 1) == 0
    assert L.gap_contigs_fit(5, TOP) == 0
    # one push: fewer than 2^32 bases including the alignment bias
    assert L.gap_push_fits(2**32 - 2, 0) == 1 and L.gap_push_fits(2**32 - 1, 0) == 1 and L.gap_push_fits(2**32, 0) == 0
    assert L.gap_push_fits(2**32 - 16, 15) == 1 and L.gap_push_fits(2**32 - 15, 15) == 0 and L.gap_push_fits(TOP, 15) == 0
    assert L.gap_push_fits(LIMIT - 1, 15) == 1


def test_standalone_program_runs_clean_under_the_sanitizers():
    """tests/genome_acc_plan_sanitize_main.cpp + the wrapper, built with AddressSanitizer and UBSan into a program of its own and run
    on the CPU: nothing is loaded into this interpreter."""
    srcs = [os.path.join(HERE, "genome_acc_plan_sanitize_main.cpp"), SRC]
    exe, stale = build_path("sylph_genome_acc_plan_sanitize", srcs + [HDR])
    if stale:
        tmp = exe + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                               "-Werror", "-o", tmp] + srcs)
        os.replace(tmp, exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "genome acc plan sanitize run ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
