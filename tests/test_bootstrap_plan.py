"""CPU tests of the bootstrap's arithmetic (sylph_amd/csrc/bootstrap_plan.h, the very header bootstrap.hip and host/inference.cpp include,
compiled with g++ through tests/bootstrap_plan_capi.cpp): position-addressed draws against a sequential WyRand + Lemire in Python ints,
the rejection flag where it can be exercised at all (n = 2^63 + 1), the summary of a histogram against ratio_lambda's choice, and the
host's split statistics against the confidence intervals recorded from the unsplit code (tests/golden/bootstrap_ci.json)."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from . import bootstrap_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def L():
    out = os.path.join(tempfile.gettempdir(), f"sylph_bootstrap_plan_{os.getuid()}.so")
    src = os.path.join(HERE, "bootstrap_plan_capi.cpp")
    hdr = os.path.join(ROOT, "sylph_amd", "csrc", "bootstrap_plan.h")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, src])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    u64, vp = C.c_uint64, C.c_void_p
    lib.bp_bins.restype = C.c_uint32
    lib.bp_summary_bytes.restype = C.c_uint32
    lib.bp_state.restype = u64
    lib.bp_state.argtypes = [u64, u64]
    lib.bp_output.restype = u64
    lib.bp_output.argtypes = [u64]
    lib.bp_draws.argtypes = [u64, u64, u64, u64, vp, vp]
    lib.bp_mul.argtypes = [u64, u64, vp, vp]
    lib.bp_values.argtypes = [vp, u64, u64, u64, vp, vp]
    lib.bp_summary.argtypes = [vp, C.c_uint32, vp]
    return lib


def plan_draws(L, seed, first, count, n):
    idx, rej = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint8)
    L.bp_draws(seed, first, count, n, idx.ctypes.data, rej.ctypes.data)
    return idx, rej


def test_constants_and_layout(L):
    assert L.bp_bins() == R.BINS >= 64 and L.bp_summary_bytes() == 4 * len(R.SUMMARY_FIELDS)
    g = R.SequentialWyRand(7)
    for j in range(5):
        out = g.next()
        assert L.bp_state(7, j) == g.s and L.bp_output(g.s) == out


def test_product_from_halves(L):
    rng = np.random.default_rng(1)
    edge = [0, 1, 0xFFFFFFFF, 0x100000000, R.M64, R.M64 - 1, 0x8000000000000000]
    pairs = [(a, b) for a in edge for b in edge] + [tuple(int(x) for x in rng.integers(0, 2**64, size=2, dtype=np.uint64)) for _ in range(2000)]
    lo, hi = C.c_uint64(), C.c_uint64()
    for a, b in pairs:
        L.bp_mul(a, b, C.byref(lo), C.byref(hi))
        assert (hi.value << 64) | lo.value == a * b, (a, b)


@pytest.mark.parametrize("n", [1, 2, 25, 255, 256, 257, 20011, 2**32 - 1])
def test_draws_equal_the_sequential_generator(L, n):
    g = R.SequentialWyRand(7)
    want = np.array([g.below(n) for _ in range(10**4)], dtype=np.uint64)
    assert not g.rejections                                            # (n / 2^64 per draw: none in 10^4)
    idx, rej = plan_draws(L, 7, 0, 10**4, n)
    assert np.array_equal(idx, want) and not rej.any()
    assert np.array_equal(R.draws(7, 0, 10**4, n), want)               # the GPU tests' numpy restatement is the same stream
    part, _ = plan_draws(L, 7, 1234, 100, n)                           # any draw on its own
    assert np.array_equal(part, want[1234:1334])


def test_rejected_is_set_exactly_where_the_sequential_generator_loops(L):
    n = 2**63 + 1                                                      # 2^64 mod n = n - 2: about half of all outputs are rejected
    g = R.SequentialWyRand(7)
    got = [g.below(n) for _ in range(2000)]
    calls = g.calls
    assert 1000 < len(g.rejections) < 3000
    idx, rej = plan_draws(L, 7, 0, calls, n)                           # position-addressed: one entry per generator call
    assert sorted(np.nonzero(rej)[0].tolist()) == g.rejections
    assert idx[rej == 0].tolist() == got                               # what is not rejected is what the generator returned, in order
    for small in (1, 2, 3, 2**32 - 1, 2**32, 2**32 + 1):               # thresholds around the 96-bit / 128-bit product seam
        g = R.SequentialWyRand(99)
        want = [g.below(small) for _ in range(500)]
        idx, rej = plan_draws(L, 99, 0, 500, small)
        assert not g.rejections and not rej.any() and idx.tolist() == want


def test_value_of_a_draw(L):
    kept = np.array([1, 1, 2, 5, 9], dtype=np.uint32)
    for n_total in (5, 6, 40):
        idx = np.arange(n_total, dtype=np.uint64)
        out = np.zeros(n_total, dtype=np.uint32)
        L.bp_values(idx.ctypes.data, n_total, n_total, len(kept), kept.ctypes.data, out.ctypes.data)
        assert out.tolist() == [0] * (n_total - len(kept)) + kept.tolist()


def plan_summary(L, hist):
    h, out = np.ascontiguousarray(hist, dtype=np.uint32), np.zeros(5, dtype=np.uint32)
    L.bp_summary(h.ctypes.data, len(h), out.ctypes.data)
    return tuple(out.tolist())


def test_summary_is_ratio_lambdas_choice(L):
    rng = np.random.default_rng(5)
    cases = [np.array([9, 0, 4, 4, 0, 3]),            # tie for the mode: the larger value (3), mode + 1 empty
             np.array([0, 7, 7, 7]),                   # three-way tie: the mode is the last bin
             np.array([5, 0, 0, 12, 0]),               # a single distinct value
             np.array([3, 0, 0, 0]),                   # nothing but zeros
             np.array([0, 2, 5, 0, 5, 1])]             # tie, the larger value has a neighbour
    for _ in range(2000):
        bins = int(rng.integers(2, R.BINS + 1))
        h = rng.integers(0, 6, size=bins) * (rng.random(bins) < rng.uniform(0.1, 1.0))
        if rng.random() < 0.3:
            h[rng.integers(1, bins)] = h.max()         # force ties
        cases.append(h)
    seen_tie = seen_single = seen_last = seen_empty_next = 0
    for h in cases:
        values = np.repeat(np.arange(len(h)), np.asarray(h, dtype=np.int64))
        want = R.summary_of_values(values)
        assert plan_summary(L, h) == want, h
        nz = np.asarray(h)[1:]
        seen_tie += int(want[3] > 0 and (nz == want[3]).sum() > 1)
        seen_single += int(want[1] == 1)
        seen_last += int(want[0] > 0 and want[2] == len(h) - 1)
        seen_empty_next += int(want[0] > 0 and want[4] == 0)
    assert min(seen_tie, seen_single, seen_last, seen_empty_next) >= 3


def test_split_statistics_give_the_recorded_intervals():
    """stats_head + bootstrap_host + finish_ci (what sylph_host_stats runs now) against the doubles the unsplit stats_from_covs gave:
    tests/golden/bootstrap_ci.json, written by tests/golden/make_bootstrap_ci.py from the commit before the split."""
    H = C.CDLL(os.path.join(ROOT, "sylph_amd", "libsylph_host.so"))
    H.sylph_host_stats.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.POINTER(R.HostStats)]
    gold = json.load(open(os.path.join(HERE, "golden", "bootstrap_ci.json")))
    vectors = R.oracle_shaped_vectors()
    assert len(vectors) == len(gold["rows"]) == 301 and gold["fields"] == ["passed", "has_ci"] + list(R.CI_FIELDS)
    with_ci = 0
    for i, ((covs, n_kmers), row) in enumerate(zip(vectors, gold["rows"])):
        cv, out = np.ascontiguousarray(covs, dtype=np.uint32), R.HostStats()
        H.sylph_host_stats(cv.ctypes.data_as(C.c_void_p), len(cv), n_kmers, 31, 3.0, 0.0, 0, 0, 0, 0, C.byref(out))
        assert [out.passed, out.has_ci] == row[:2], i
        for f, want in zip(R.CI_FIELDS, row[2:]):
            assert getattr(out, f) == float.fromhex(want), (i, f)
        with_ci += out.has_ci
    assert with_ci > 100 and gold["rows"][-1][1] == 1


def test_standalone_program_runs_clean_under_the_sanitizers():
    """tests/bootstrap_sanitize_main.cpp + host/inference.cpp (which includes the plan), built with AddressSanitizer and UBSan into a
    program of its own and run on the CPU: nothing is loaded into this interpreter, nothing runs on a GPU."""
    exe = os.path.join(tempfile.gettempdir(), f"sylph_bootstrap_sanitize_{os.getuid()}")
    srcs = [os.path.join(HERE, "bootstrap_sanitize_main.cpp"), os.path.join(ROOT, "sylph_amd", "host", "inference.cpp")]
    deps = srcs + [os.path.join(ROOT, "sylph_amd", "host", "sylph_host.hpp"), os.path.join(ROOT, "sylph_amd", "csrc", "bootstrap_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        tmp = exe + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                               "-Werror", "-o", tmp] + srcs)
        os.replace(tmp, exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "bootstrap sanitize run ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
