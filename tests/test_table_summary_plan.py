"""CPU tests of K15's arithmetic (sylph_amd/csrc/table_summary_plan.h, the very header table_summary.hip includes, compiled with g++
through tests/table_summary_plan_capi.cpp): the three lemmas the parallel walk rests on by brute force, the sequential model of
passes 1-3 against the plain walk and against oracle/pyref.py, the wrap, the declines, the ladder."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from hypothesis import given, settings
from hypothesis import strategies as st

from oracle import pyref as P

from . import table_summary_ref as T
from .helpers import build_path

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "table_summary_plan_capi.cpp")
HDR = os.path.join(ROOT, "sylph_amd", "csrc", "table_summary_plan.h")


class RungState(C.Structure):
    _fields_ = [("median_sum", C.c_uint64), ("total_counts", C.c_uint64)] + [(f, C.c_uint32) for f in ("steps", "num_1s", "num_not1s", "max_state", "gave_up", "open")]


def load_plan():
    out, stale = build_path("sylph_table_summary_plan", [SRC, HDR], ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, SRC])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.ts_constants.argtypes = [vp]
    lib.ts_step.restype = u32
    lib.ts_step.argtypes = [u32, u32]
    lib.ts_ladder_ok.argtypes = [vp, vp, u32, u32]
    lib.ts_walk.argtypes = [vp, u64, C.POINTER(T.Summary)]
    lib.ts_model.argtypes = [vp, u64, vp, vp, u32, u32, C.POINTER(T.Summary)]
    lib.ts_finish.argtypes = [vp, vp, vp, u32, u64, C.POINTER(T.Summary)]
    lib.ts_lemmas.argtypes = [u32, u32, u32, u32, vp]
    return lib


@pytest.fixture(scope="module")
def L():
    return load_plan()


def constants(L):
    out = np.zeros(20, dtype=np.uint32)
    L.ts_constants(out.ctypes.data)
    o = out.tolist()
    n_rungs = o[10]
    return dict(max_rungs=o[0], group=o[1], tile=o[2], sizes=o[3:6], flags=o[6:10], n_rungs=n_rungs, max_open=o[11],
                caps=o[12:12 + 2 * n_rungs:2], chunks=o[13:13 + 2 * n_rungs:2])


def model(L, counts, caps, chunks, max_open=64):
    a = np.ascontiguousarray(counts, dtype=np.uint32)
    caps, chunks = np.asarray(caps, dtype=np.uint32), np.asarray(chunks, dtype=np.uint32)
    s = T.Summary()
    assert L.ts_model(a.ctypes.data, len(a), caps.ctypes.data, chunks.ctypes.data, len(caps), max_open, C.byref(s)) == 0
    return s.as_dict()


def plain(L, counts):
    a = np.ascontiguousarray(counts, dtype=np.uint32)
    s = T.Summary()
    L.ts_walk(a.ctypes.data, len(a), C.byref(s))
    return s.as_dict()


def walk_fields(d):
    return {f: d[f] for f in T.WALK_FIELDS}


def test_constants_and_layout(L):
    k = constants(L)
    assert k["sizes"] == [C.sizeof(T.Summary), C.sizeof(RungState), 12] and C.sizeof(T.Summary) == 48 and C.sizeof(RungState) == 40
    assert k["flags"] == [T.DECLINED, T.DECLINED_LADDER, T.DECLINED_SUM, T.DECLINED_SIZE]
    assert 1 <= k["n_rungs"] <= k["max_rungs"] == 4 and k["group"] == 64
    assert k["caps"] == sorted(set(k["caps"])) and min(k["caps"]) >= 2
    from sylph_amd import binding
    assert binding.TABLE_SUMMARY.itemsize == 48 and binding.TABLE_SUMMARY.names == T.FIELDS


def test_the_three_lemmas_by_brute_force(L):
    """every count vector over {0..6} of length 0..7, every same-parity pair of start states up to 9, every cap 2..8"""
    out = np.zeros(8, dtype=np.uint64)
    L.ts_lemmas(6, 7, 9, 8, out.ctypes.data)
    assert int(out[0]) == sum(7 ** n for n in range(8))
    assert out[1:].tolist() == [0] * 7, dict(zip(("parity", "order", "shrink", "stay_equal", "clamp_bound", "clamp_identity", "wrap"), out[1:].tolist()))


def test_the_lemmas_in_python_on_a_smaller_domain():
    """the same statements written out here, over {0..4}^(<=5): the C enumeration above is not the only witness"""
    import itertools
    step = lambda m, x: m + 1 if x > m else m - 1
    for n in range(6):
        for v in itertools.product(range(5), repeat=n):
            xs = [x for x in v if x > 1]
            m = 0
            for i, x in enumerate(xs, 1):
                m = step(m, x)
                assert m % 2 == i % 2 and m >= 1
            for a in range(7):
                for b in range(a, 7, 2):
                    p, q = a, b
                    for x in xs:
                        d, between = q - p, p < x <= q
                        p, q = step(p, x), step(q, x)
                        assert p <= q and q - p == (d - 2 if between else d)
            for cap in (2, 3, 4):
                m = mc = 0
                same, reached = True, False
                for x in xs:
                    m, mc = step(m, x), step(mc, min(x, cap))
                    assert mc <= cap
                    reached |= mc >= cap
                    same &= m == mc
                assert reached or same


def test_step_and_plain_walk_equal_the_restatement(L):
    rng = np.random.default_rng(1)
    assert [L.ts_step(m, x) for m, x in ((0, 2), (1, 2), (2, 2), (5, 2**32 - 1), (7, 3))] == [1, 2, 1, 6, 6]
    for n in (0, 1, 2, 50, 3000):
        for lam in (0.3, 2.5, 40.0):
            c = rng.poisson(lam, size=n).astype(np.uint32)
            assert walk_fields(plain(L, c)) == T.walk(c)


@settings(max_examples=300, deadline=None)
@given(st.lists(st.one_of(st.integers(0, 9), st.integers(0, 40), st.sampled_from([2**31, 2**32 - 1, 10**6])), max_size=300),
       st.sampled_from([((2,), (1,)), ((4, 16), (8, 8)), ((3, 5, 64), (2, 7, 33)), ((64,), (32,)), ((8, 4096), (65, 31))]),
       st.sampled_from([0, 1, 3, 64]), st.sampled_from([21, 31]), st.sampled_from([150.0, 1000.0]))
def test_model_equals_the_plain_walk_and_pyref(counts, ladder, max_open, k, mean_len):
    """tiny caps and chunks: whatever the model answers is the plain walk, field for field; what it declines it flags; and the f64
    values the host derives from the integers are pyref's, bit for bit"""
    L = load_plan()
    caps, chunks = ladder
    got, want = model(L, counts, caps, chunks, max_open), T.walk(counts)
    for f in ("total_counts", "steps", "num_1s", "num_not1s"):
        assert got[f] == want[f], f
    if got["flags"] & T.DECLINED:
        assert got["flags"] == T.DECLINED | T.DECLINED_LADDER and got["rung"] == len(caps) and got["median_sum"] == 0 and got["max_state"] == 0
        return
    assert got["flags"] == 0 and walk_fields(got) == want and want["max_state"] < caps[got["rung"]]
    # the host's tail, restated: the decision pyref takes from the counts == the one taken from the integers
    med = T.mov_avg_median(got)
    eps = float(got["num_not1s"]) / (float(got["num_not1s"]) + float(got["num_1s"]) + 0.1)
    from_summary = 0.995 ** float(k) if (med < P.MED_KMER_FOR_ID_EST and mean_len < 400.0) else (eps if eps < 1.0 else 1.0)
    assert from_summary == P.get_kmer_identity(counts, k, mean_len)


def test_a_cap_the_walk_reaches_is_refused_and_the_next_rung_answers(L):
    c = np.full(200, 50, dtype=np.uint32)                       # the state climbs to 50
    s = model(L, c, (4, 16, 64), (8, 8, 64))
    assert s["rung"] == 2 and s["flags"] == 0 and walk_fields(s) == T.walk(c)
    assert s["max_state"] == 50
    c = np.full(200, 16, dtype=np.uint32)                       # reaches 16 exactly: max_state < C fails at C = 16
    assert model(L, c, (4, 16, 64), (8, 8, 64))["rung"] == 2
    c = np.full(200, 15, dtype=np.uint32)
    assert model(L, c, (4, 16, 64), (8, 8, 64))["rung"] == 1


def test_ladder_exhaustion_and_max_open(L):
    never = np.tile(np.array([2, 10**6], dtype=np.uint32), 500)  # alternates down / up: the two walks never meet
    s = model(L, never, (4, 16), (8, 8))
    assert s["flags"] == T.DECLINED | T.DECLINED_LADDER and s["rung"] == 2
    assert {f: s[f] for f in ("total_counts", "steps", "num_1s", "num_not1s")} == {f: T.walk(never)[f] for f in ("total_counts", "steps", "num_1s", "num_not1s")}
    # with a chunk that holds the whole table nothing is open: the plain walk stays at 1, 2, 1, 2 ..
    s = model(L, never, (4, 16), (1000, 1000))
    assert s["flags"] == 0 and s["rung"] == 0 and s["open_chunks"] == 1 and walk_fields(s) == T.walk(never)
    # open chunks are walked again up to max_open of them, not one more
    c = np.tile(np.array([2, 3], dtype=np.uint32), 64)           # 16 chunks of 8, every one open at cap 16
    assert model(L, c, (16,), (8,), max_open=16)["open_chunks"] == 16
    assert model(L, c, (16,), (8,), max_open=16)["flags"] == 0
    assert model(L, c, (16,), (8,), max_open=15)["flags"] == T.DECLINED | T.DECLINED_LADDER
    for bad in (((1,), (8,)), ((4, 4), (8, 8)), ((16, 4), (8, 8)), ((4,), (0,)), ((2**30 + 1,), (8,)), ((), ()), ((2, 3, 4, 5, 6), (1,) * 5)):
        caps, chunks = (np.asarray(x, dtype=np.uint32) for x in bad)
        assert L.ts_ladder_ok(caps.ctypes.data, chunks.ctypes.data, len(caps), 64) == 0, bad


def test_wrap_zeros_ones_and_empty_chunks(L):
    two = np.array([2**31, 2**31], dtype=np.uint32)
    s = model(L, two, (4, 16), (8, 8))
    assert s["num_not1s"] == 0 and s["total_counts"] == 2**32 and s["steps"] == 2 and s["median_sum"] == 3 and walk_fields(s) == T.walk(two)
    zeros = np.array([0, 0, 5, 0, 1, 0, 7, 0], dtype=np.uint32)  # a count of 0 is no step, adds nothing, and is not a 1
    s = model(L, zeros, (4, 16), (3, 3))
    assert s["steps"] == 2 and s["num_1s"] == 1 and s["num_not1s"] == 12 and walk_fields(s) == T.walk(zeros)
    ones = np.ones(1000, dtype=np.uint32)                        # no step anywhere: no chunk is open, nothing declines
    s = model(L, ones, (4, 16), (8, 8), max_open=0)
    assert s["flags"] == 0 and s["steps"] == 0 and s["num_1s"] == 1000 and s["open_chunks"] == 0 and s["median_sum"] == 0
    middle = np.concatenate([np.full(24, 3), np.ones(16), np.full(24, 3)]).astype(np.uint32)      # chunks 3 and 4 of 8 hold no step
    s = model(L, middle, (4, 16), (8, 8), max_open=0)
    assert s["flags"] == 0 and walk_fields(s) == T.walk(middle)
    assert model(L, [], (4, 16), (8, 8)) == dict.fromkeys(T.FIELDS, 0)


def test_the_2_53_decline_and_the_size_decline(L):
    caps, chunks = np.array([64, 1024], dtype=np.uint32), np.array([4096, 16384], dtype=np.uint32)
    def finish(states, n):
        arr = (RungState * 2)(*states)
        s = T.Summary()
        assert L.ts_finish(arr, caps.ctypes.data, chunks.ctypes.data, 2, n, C.byref(s)) == 0
        return s.as_dict()
    ok = RungState(2**53 - 1, 99, 2**31 - 1, 5, 6, 63, 0, 0)     # forged: no table gets there
    s = finish([ok, RungState()], 2**31 - 1)
    assert s["flags"] == 0 and s["median_sum"] == 2**53 - 1 and s["rung"] == 0 and float(s["median_sum"]) == 2.0**53 - 1
    big = RungState(2**53, 99, 2**31 - 1, 5, 6, 63, 0, 0)
    s = finish([big, RungState()], 2**31 - 1)
    assert s["flags"] == T.DECLINED | T.DECLINED_SUM and s["median_sum"] == 0 and s["steps"] == 2**31 - 1 and s["num_not1s"] == 6
    first_fails = RungState(7, 99, 10, 5, 6, 64, 0, 0)           # max_state == cap: rung 0 is refused, rung 1 answers
    s = finish([first_fails, RungState(77, 99, 10, 5, 6, 70, 0, 3)], 100)
    assert s["flags"] == 0 and s["rung"] == 1 and s["median_sum"] == 77 and s["open_chunks"] == 3
    s = finish([first_fails, RungState(77, 99, 10, 5, 6, 70, 1, 3)], 100)
    assert s["flags"] == T.DECLINED | T.DECLINED_LADDER
    s = finish([ok, ok], 2**31)
    assert s["flags"] == T.DECLINED | T.DECLINED_SIZE and s["steps"] == 0


def test_default_ladder_on_simulated_tables(L):
    """the issue's simulation, re-run for the defaults chosen here: no decline, and the rung each family answers on"""
    k = constants(L)
    rungs = {}
    for name, seed, depth, ones in T.FAMILIES:
        c = T.family(seed, depth, ones=ones)
        s = model(L, c, k["caps"], k["chunks"], k["max_open"])
        assert s["flags"] == 0 and walk_fields(s) == walk_fields(plain(L, c)), name
        rungs[name] = (s["rung"], s["open_chunks"], round(T.mov_avg_median(s)))
    assert rungs["near3"][0] == 0 and rungs["near9"][0] == 0 and rungs["near400"][0] == 1, rungs
    assert abs(rungs["near3"][2] - 3) <= 1 and abs(rungs["near9"][2] - 9) <= 2 and abs(rungs["near400"][2] - 400) <= 60, rungs
    assert max(r[1] for r in rungs.values()) <= 2, rungs


def test_standalone_program_runs_clean_under_the_sanitizers():
    """tests/table_summary_sanitize_main.cpp + the model, built with AddressSanitizer and UBSan into a program of its own and run on the
    CPU: nothing is loaded into this interpreter, nothing runs on a GPU."""
    srcs = [os.path.join(HERE, "table_summary_sanitize_main.cpp"), SRC]
    exe, stale = build_path("sylph_table_summary_sanitize", srcs + [HDR])
    if stale:
        tmp = exe + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                               "-Werror", "-o", tmp] + srcs)
        os.replace(tmp, exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "table summary sanitize run ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    assert " 0 tables" not in p.stdout and " 0 declined" not in p.stdout and " 0 later-rung" not in p.stdout
