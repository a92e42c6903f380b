"""CPU tests of the statistics head's integer half (sylph_amd/csrc/row_stats_plan.h, the very header row_stats.hip and host/inference.cpp
include, compiled with g++ through tests/row_stats_plan_capi.cpp): the summary of a row against a numpy restatement of contain.rs /
inference.rs, the host's split statistics against the unsplit entry field for field, the table behind the Poisson cut and the
monotony it rests on, the kernel's work split replayed lane by lane, and the soundness of the conservative reject."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from . import bootstrap_ref as R
from . import row_stats_ref as RS
from .helpers import build_path

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "row_stats_plan_capi.cpp")
HDR = os.path.join(ROOT, "sylph_amd", "csrc", "row_stats_plan.h")
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32}
# (minimum_ani_or_neg, pseudotax, no_adj, mean_coverage): profile, query, -m 80, --no-adjust, --mean-coverage
CONFIGS = {"profile": (-1.0, 1, 0, 0), "query": (-1.0, 0, 0, 0), "m80": (80.0, 1, 0, 0), "no_adjust": (-1.0, 1, 1, 0), "mean_coverage": (-1.0, 0, 0, 1)}
STAT_FIELDS = [f for f, _ in R.HostStats._fields_ if f != "pad"]


@pytest.fixture(scope="module")
def L():
    out, stale = build_path("sylph_row_stats_plan", [SRC, HDR], ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, SRC])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.rs_constants.argtypes = [vp]
    lib.rs_keep_limit.restype = u32
    lib.rs_keep_limit.argtypes = [u32, vp]
    lib.rs_summarise.argtypes = [vp, u32, u32, vp, vp]
    lib.rs_replay.argtypes = [vp, u32, u32, vp, vp]
    lib.rs_cut_table.argtypes = [vp, u32, vp]
    lib.rs_surely_rejected.argtypes = [vp, u32, u64, vp]
    lib.rs_surely_rejected_n.argtypes = [vp, vp, u64, vp, vp]
    return lib


@pytest.fixture(scope="module")
def H():
    h = RS.host_lib()
    h.sylph_host_row_cut_table.argtypes = [C.c_void_p]
    h.sylph_host_row_cut_table.restype = None
    h.sylph_host_row_filter.argtypes = [C.c_uint64, C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(RS.RowFilter)]
    h.sylph_host_row_filter.restype = None
    h.sylph_host_stats_from_summary.argtypes = [C.POINTER(RS.RowSummary), C.c_void_p, C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_int, C.c_int,
                                                C.c_int, C.c_int, C.POINTER(R.HostStats)]
    return h


@pytest.fixture(scope="module")
def cut(H):
    t = np.zeros(RS.CUT_ENTRIES, dtype=np.uint32)
    H.sylph_host_row_cut_table(t.ctypes.data)
    return t


def plan_summary(L, row, cut, width=None, fn="rs_summarise"):
    width = width or RS.width_of(row)
    a, out = np.ascontiguousarray(row, dtype=DTYPE[width]), np.zeros(9, dtype=np.uint32)
    assert getattr(L, fn)(a.ctypes.data, width, len(a), cut.ctypes.data, out.ctypes.data) == 0
    return dict(zip(RS.FIELDS[1:], out.tolist()[1:]))


def random_rows(rng, n):
    rows = []
    for i in range(n):
        length = int(rng.choice([1, 2, 5, 24, 25, 26, 60, 64, 65, 200, 700])) if i % 3 else int(rng.integers(1, 400))
        lam = float(rng.choice([0.05, 0.4, 1.0, 2.0, 3.5, 12.0, 28.0, 45.0]))
        row = rng.poisson(lam, size=length).astype(np.uint64) + np.uint64(1)
        if i % 9 == 0:
            row[rng.integers(0, length, size=min(3, length))] = int(rng.choice([200, 70000, 1 << 31]))      # outliers the cut drops
        rows.append(np.sort(row))
    return rows


def test_constants_and_layout(L):
    out = np.zeros(7, dtype=np.uint32)
    L.rs_constants(out.ctypes.data)
    assert out.tolist() == [RS.CUT_ENTRIES, RS.CUT_NONE, 64, int(RS.MEDIAN_ANI_THRESHOLD), RS.SAMPLE_SIZE_CUTOFF, C.sizeof(RS.RowFilter),
                            C.sizeof(RS.RowSummary)]
    assert C.sizeof(RS.RowFilter) == 152 and C.sizeof(RS.RowSummary) == 36
    from sylph_amd import binding
    assert C.sizeof(binding.RowFilter) == 152 and binding.ROW_SUMMARY.itemsize == 36 and binding.ROW_SUMMARY.names == RS.FIELDS


def test_cdf_is_monotone_and_the_table_is_its_first_failure(L, H, cut):
    """The table equals the reference's loop over the values present only if the cdf does not decrease in x: m = 1..29, x = 0..200."""
    cdf = RS.host_cdf(H)
    for m in range(1, 30):
        vals = [cdf(m, x) for x in range(201)]
        assert all(b >= a for a, b in zip(vals, vals[1:])), m
        assert cut[m] != RS.CUT_NONE and m <= cut[m] < 200, (m, cut[m])
        assert all((v < RS.CUTOFF_PVALUE) == (x <= cut[m]) for x, v in enumerate(vals) if x >= m), m
    assert cut.tolist() == RS.cut_table(cdf)                                   # the host's table is the definition's
    assert cut[0] == RS.CUT_NONE                                               # cdf(0, 0) = 1
    stride = 202
    ok = np.array([[1 if cdf(m, x) < RS.CUTOFF_PVALUE else 0 for x in range(stride)] for m in range(30)], dtype=np.uint8)
    t = np.zeros(30, dtype=np.uint32)
    L.rs_cut_table(ok.ctypes.data, stride, t.ctypes.data)                      # build_cut_table from the same answers
    assert t.tolist() == cut.tolist()
    for m in (0, 1, 29, 30, 31, 1000):
        want = 0xFFFFFFFF if m >= 30 or cut[m] == RS.CUT_NONE else int(cut[m])
        assert L.rs_keep_limit(m, cut.ctypes.data) == want


def all_rows(cut):
    rows = dict(RS.crafted_rows())
    rows.update(RS.cut_rows(cut))
    rows.update({f"random{i}": r for i, r in enumerate(random_rows(np.random.default_rng(4), 600))})
    return rows


def test_summary_equals_the_restatement_and_the_replay_equals_the_summary(L, H, cut):
    cdf = RS.host_cdf(H)
    rows = all_rows(cut)
    seen = dict(cut=0, wrap=0, tie=0, single=0, no_next=0, long=0)
    for name, row in rows.items():
        want = RS.summary_of_row(row, cdf)
        for width in sorted({RS.width_of(row), 4}):
            assert plan_summary(L, row, cut, width) == want, (name, width)
            assert plan_summary(L, row, cut, width, "rs_replay") == want, (name, width)
        seen["cut"] += want["keep"] < len(row)
        seen["wrap"] += int(np.sum(row[:want["keep"]], dtype=np.uint64)) >= 1 << 32
        seen["single"] += want["n_distinct"] == 1
        seen["no_next"] += want["next_count"] == 0
        seen["long"] += len(row) > 128
        vals, cnt = np.unique(row[:want["keep"]], return_counts=True)
        seen["tie"] += int((cnt == cnt.max()).sum() > 1)
    assert min(seen.values()) >= 2, seen
    s = RS.summary_of_row(rows["next_beyond_cut"], cdf)
    assert s["median"] == 3 and s["mode"] == cut[3] and s["next_count"] == 0 and s["keep"] == 29
    for m in (1, 2, 3, 29):
        s = RS.summary_of_row(rows[f"cut_at_median{m}"], cdf)
        assert s["median"] == m and s["keep"] == 48
    assert RS.summary_of_row(rows["median30"], cdf)["keep"] == 59
    assert RS.summary_of_row(rows["sum_wraps"], cdf)["sum"] == (3 << 31) & 0xFFFFFFFF


def host_stats(H, row, n_kmers, cfg, no_ci):
    min_ani, pseudotax, no_adj, mean_cov = CONFIGS[cfg]
    cv, out = np.ascontiguousarray(row, dtype=np.uint32), R.HostStats()
    H.sylph_host_stats(cv.ctypes.data, len(cv), n_kmers, 31, 3.0, min_ani, pseudotax, no_ci, no_adj, mean_cov, C.byref(out))
    return out


def test_statistics_from_a_summary_equal_the_statistics_from_the_row(L, H, cut):
    """sylph_host_stats_from_summary(summary) == sylph_host_stats(row), field for field, == on doubles"""
    rng = np.random.default_rng(9)
    rows = all_rows(cut)
    passed = with_ci = 0
    for i, (name, row) in enumerate(rows.items()):
        s = plan_summary(L, row, cut)
        rs = RS.RowSummary(0, *[s[f] for f in RS.FIELDS[1:]])
        cv = np.ascontiguousarray(row, dtype=np.uint32)
        n_kmers = len(row) + int(rng.choice([0, 1, len(row) // 3, 3 * len(row), 40 * len(row)]))
        for cfg, (min_ani, pseudotax, no_adj, mean_cov) in CONFIGS.items():
            no_ci = 0 if (i % 16 == 0 and len(row) < 300) else 1
            want, got = host_stats(H, row, n_kmers, cfg, no_ci), R.HostStats()
            H.sylph_host_stats_from_summary(C.byref(rs), cv.ctypes.data, n_kmers, 31, 3.0, min_ani, pseudotax, no_ci, no_adj, mean_cov, C.byref(got))
            for f in STAT_FIELDS:
                assert getattr(got, f) == getattr(want, f), (name, cfg, f)
            passed += want.passed
            with_ci += want.has_ci
    assert passed > 200 and with_ci >= 3


def soundness_rows(rng, n):
    """rows around the ANI cuts: genomes of 60-800 k-mers hit at an ANI between 0.80 and 1, Poisson coverages; and rows of ones whose
    containment lies at the cut itself, one above and one below"""
    n_kmers = rng.integers(60, 800, size=n)
    ani = rng.uniform(0.80, 1.0, size=n)
    contain = np.maximum(1, rng.binomial(n_kmers, ani ** 31))
    lam = rng.choice([0.05, 0.3, 0.8, 1.5, 3.0, 10.0], size=n)
    for j in range(0, n, 50):                                                  # at the cut
        min_ani = (0.95, 0.9, 0.8)[(j // 50) % 3]
        contain[j] = min(n_kmers[j], max(1, int(np.ceil(min_ani ** 31 * n_kmers[j])) + int(rng.integers(-1, 2))))
        lam[j] = 0.0
    vals = rng.poisson(np.repeat(lam, contain)).astype(np.uint32)
    vals[vals == 0] = 1
    off = np.concatenate([[0], np.cumsum(contain)])
    return n_kmers, off, vals


def test_no_accepted_row_is_surely_rejected(L, H, cut):
    """Soundness over 10^5 random rows: what stats_head accepts, surely_rejected keeps.  Allowed exceptions: 0."""
    rng = np.random.default_rng(17)
    N = 100_000
    n_kmers, off, vals = soundness_rows(rng, N)
    cfgs = ["profile", "query", "m80", "no_adjust"]
    summaries = np.zeros((N, 9), dtype=np.uint32)
    accepted, lam_status = np.zeros(N, dtype=bool), np.zeros(N, dtype=np.int64)
    out = R.HostStats()
    for i in range(N):
        row = np.sort(vals[off[i]:off[i + 1]])
        min_ani, pseudotax, no_adj, mean_cov = CONFIGS[cfgs[i % 4]]
        H.sylph_host_stats(row.ctypes.data, len(row), int(n_kmers[i]), 31, 3.0, min_ani, pseudotax, 1, no_adj, mean_cov, C.byref(out))
        accepted[i], lam_status[i] = out.passed, out.lambda_status
        assert L.rs_summarise(row.ctypes.data, 4, len(row), cut.ctypes.data, summaries[i].ctypes.data) == 0
    # the inputs hold, by the host's unsplit statistics alone, accepted and rejected rows, and accepted rows with and without a lambda
    assert accepted.sum() > 1000 and (~accepted).sum() > 1000
    assert (accepted & (lam_status == 2)).sum() > 100 and (accepted & (lam_status != 2)).sum() > 100
    dropped = np.zeros(N, dtype=np.uint8)
    for c, cfg in enumerate(cfgs):
        min_ani, pseudotax, no_adj, _ = CONFIGS[cfg]
        f = RS.RowFilter()
        H.sylph_host_row_filter(31, 3.0, min_ani, pseudotax, no_adj, C.byref(f))
        assert f.struct_size == C.sizeof(f) and f.k == 31 and list(f.cut) == cut.tolist() and f.no_adj == no_adj
        want_ani = min_ani / 100 if min_ani >= 0 else (0.95 if pseudotax else 0.9)
        assert f.reject_below == want_ani ** 31 * (1 - 2.0 ** -30)
        sel = np.arange(c, N, 4)
        part = np.ascontiguousarray(summaries[sel])
        nk = np.ascontiguousarray(n_kmers[sel], dtype=np.uint64)
        res = np.zeros(len(sel), dtype=np.uint8)
        L.rs_surely_rejected_n(part.ctypes.data, nk.ctypes.data, len(sel), C.byref(f), res.ctypes.data)
        dropped[sel] = res
    exceptions = int((accepted & (dropped != 0)).sum())
    assert exceptions == 0
    assert dropped.sum() > 1000                                                # the filter does drop rows
    # what it lets through without need is the band below the cut and nothing else to speak of
    assert (~accepted & (dropped == 0)).sum() < 0.01 * N


def test_reject_below_zero_keeps_everything(L, H):
    f = RS.RowFilter()
    H.sylph_host_row_filter(31, 3.0, 0.0, 0, 0, C.byref(f))
    assert f.reject_below == 0.0
    s = np.array([0, 1, 1, 1, 1, 1, 1, 1, 0], dtype=np.uint32)
    assert L.rs_surely_rejected(s.ctypes.data, 1, 10**9, C.byref(f)) == 0
    H.sylph_host_row_filter(31, 3.0, -1.0, 1, 0, C.byref(f))
    assert L.rs_surely_rejected(s.ctypes.data, 1, 10**9, C.byref(f)) == 1
    # an infinite lambda (a mode count of 0 cannot come from a row; min_count_correct 0 lets it through): exp(-inf) = 0, the index is
    # keep / n_total, finite, and far below the cut
    f.min_count_correct = 0.0
    odd = np.array([0, 30, 1, 30, 30, 2, 1, 0, 3], dtype=np.uint32)
    assert L.rs_surely_rejected(odd.ctypes.data, 30, 10**9, C.byref(f)) == 1


def test_standalone_program_runs_clean_under_the_sanitizers():
    """tests/row_stats_sanitize_main.cpp + the replay + host/inference.cpp, built with AddressSanitizer and UBSan into a program of its
    own and run on the CPU: nothing is loaded into this interpreter, nothing runs on a GPU."""
    srcs = [os.path.join(HERE, "row_stats_sanitize_main.cpp"), SRC, os.path.join(ROOT, "sylph_amd", "host", "inference.cpp")]
    deps = srcs + [HDR, os.path.join(ROOT, "sylph_amd", "host", "sylph_host.hpp"), os.path.join(ROOT, "sylph_amd", "csrc", "bootstrap_plan.h")]
    exe, stale = build_path("sylph_row_stats_sanitize", deps)
    if stale:
        tmp = exe + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                               "-Werror", "-o", tmp] + srcs)
        os.replace(tmp, exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "row stats sanitize run ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    assert " 0 rows" not in p.stdout and " 0 cut" not in p.stdout and " 0 long" not in p.stdout
