"""What the row-statistics tests share (tests/test_row_stats_plan.py, tests/test_gpu_row_stats.py): the integers the statistics head
reads off a coverage row, restated in numpy from contain.rs:661-690 and inference.rs:207-242 — the loop over the values that are
present, not the table of csrc/row_stats_plan.h —, ratio_lambda's decision, the containment index, and the rows the tests run.
Nothing here calls the code under test; the Poisson cdf is handed in (the host's own, which is what the cut is defined by)."""
import ctypes as C
import os

import numpy as np

from . import bootstrap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTOFF_PVALUE = 0.9999999999
SAMPLE_SIZE_CUTOFF, MEDIAN_ANI_THRESHOLD = 25, 2.0
CUT_ENTRIES, CUT_NONE = 30, 0xFFFFFFFF
FIELDS = ("row", "contain_count", "median", "keep", "sum", "n_distinct", "mode", "mode_count", "next_count")


class RowSummary(C.Structure):          # sylph_row_summary
    _fields_ = [(f, C.c_uint32) for f in FIELDS]


class RowFilter(C.Structure):           # sylph_row_filter
    _fields_ = [("struct_size", C.c_uint32), ("k", C.c_uint32), ("reject_below", C.c_double), ("min_count_correct", C.c_double),
                ("no_adj", C.c_uint32), ("reserved", C.c_uint32), ("cut", C.c_uint32 * CUT_ENTRIES)]


def host_lib():
    """libsylph_host.so with the entry points the row-statistics tests call"""
    H = C.CDLL(os.path.join(ROOT, "sylph_amd", "libsylph_host.so"))
    H.sylph_host_poisson_cdf.restype = C.c_double
    H.sylph_host_poisson_cdf.argtypes = [C.c_double, C.c_uint64]
    H.sylph_host_stats.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.POINTER(R.HostStats)]
    return H


def host_cdf(H):
    memo = {}

    def cdf(m, x):
        if (m, x) not in memo:
            memo[(m, x)] = H.sylph_host_poisson_cdf(float(m), int(x))
        return memo[(m, x)]
    return cdf


def cut_table(cdf):
    """cut[m], m < 30: the largest x with cdf(m, y) < CUTOFF_PVALUE for every integer y in [m, x]; CUT_NONE if cdf(m, m) fails already"""
    cut = []
    for m in range(CUT_ENTRIES):
        if not cdf(m, m) < CUTOFF_PVALUE:
            cut.append(CUT_NONE)
            continue
        x = m
        while cdf(m, x + 1) < CUTOFF_PVALUE:
            x += 1
        cut.append(x)
    return cut


def summary_of_row(row, cdf):
    """-> dict of FIELDS[1:] for a row of coverage values (any order), as get_stats reads it"""
    covs = np.sort(np.asarray(row, dtype=np.uint64))                          # :661
    n = len(covs)
    median = int(covs[n // 2])                                                # :663
    max_cov = None                                                            # f64::MAX
    if median < 30:                                                           # :666-675
        for v in covs[n // 2:].tolist():
            if cdf(median, v) < CUTOFF_PVALUE:
                max_cov = v
            else:
                break
    kept = covs if max_cov is None else covs[covs <= np.uint64(max_cov)]      # :679-684 without the zeros
    n_nonzero, n_distinct, mode, mode_count, next_count = R.summary_of_values(kept)
    assert n_nonzero == len(kept)
    return dict(contain_count=n, median=median, keep=len(kept), sum=int(kept.sum(dtype=np.uint64)) & 0xFFFFFFFF,   # iter().sum::<u32>()
                n_distinct=n_distinct, mode=mode, mode_count=mode_count, next_count=next_count)


def lambda_of(s, min_count_correct):
    """ratio_lambda (inference.rs:207-242) behind the median test of contain.rs:693, from a summary; None: no lambda"""
    if s["median"] > MEDIAN_ANI_THRESHOLD:
        return None
    if s["n_distinct"] == 1 or s["keep"] < SAMPLE_SIZE_CUTOFF or s["next_count"] == 0:
        return None
    if s["next_count"] < min_count_correct or s["mode_count"] < min_count_correct:
        return None
    return s["next_count"] / s["mode_count"] * float(s["mode"] + 1)


def containment_index(s, n_genome_kmers, min_count_correct, no_adj):
    """what contain.rs:657-660 / :817-847 take the k-th root of (the lambda path's exp is this interpreter's libm)"""
    lam = None if no_adj else lambda_of(s, min_count_correct)
    if lam is None:
        return s["contain_count"] / n_genome_kmers
    return s["keep"] / (1.0 - np.exp(-lam)) / (n_genome_kmers - s["contain_count"] + s["keep"])


def run_row(pairs):
    """[(value, times), ...] -> the row"""
    return np.concatenate([np.full(t, v, dtype=np.uint64) for v, t in pairs])


def crafted_rows():
    """name -> ascending row (uint64 values; every one fits 32 bits)"""
    rng = np.random.default_rng(21)
    rows = {}
    for n in (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257):
        rows[f"len{n}"] = np.sort(rng.poisson(1.3, size=n).astype(np.uint64) + np.uint64(1))
    long_ = rng.poisson(1.1, size=9000)
    rows["len5000"] = np.sort(long_[long_ > 0][:5000].astype(np.uint64))
    rows["all_equal"] = run_row([(2, 40)])
    rows["run_crosses_chunk"] = run_row([(1, 50), (2, 30), (3, 10)])                   # the run of 2 lies over values 50..79
    rows["run_spans_three_chunks"] = run_row([(1, 40), (2, 150), (3, 20)])             # 40..189: chunks 0, 1 and 2
    rows["tie_goes_up"] = run_row([(1, 20), (2, 20), (3, 5)])
    rows["tie_across_chunks"] = run_row([(1, 70), (2, 70), (3, 10)])
    rows["next_absent"] = run_row([(1, 10), (2, 30), (4, 12)])
    rows["w8_edge"] = run_row([(1, 30), (255, 2)])
    rows["w16_lo"] = run_row([(1, 30), (255, 1), (256, 2)])
    rows["w16_edge"] = run_row([(1, 30), (65535, 2)])
    rows["w32_lo"] = run_row([(1, 30), (65535, 1), (65536, 2)])
    rows["sum_wraps"] = run_row([(1 << 31, 3)])
    rows["sum_wraps_long"] = run_row([(7, 100), (1 << 31, 3)])                         # median 7 has a cut: the big values go
    rows["high_median"] = np.sort(rng.integers(40, 90, size=300).astype(np.uint64))
    rows["max_value"] = run_row([(0xFFFFFFFE, 3), (0xFFFFFFFF, 4)])
    return rows


def cut_rows(cut):
    """rows whose cut falls inside a run's value range, at medians 1, 2, 3, 29 (the cut's own value present, the next one too) and 30
    (no cut); and one where mode + 1 is present but lies beyond the cut"""
    rows = {}
    for m in (1, 2, 3, 29):
        c = int(cut[m])
        assert c != CUT_NONE and c >= m
        rows[f"cut_at_median{m}"] = run_row([(m, 41), (c, 7), (c + 1, 9), (c + 50, 2)])
        rows[f"cut_long_median{m}"] = run_row([(m, 141), (c, 70), (c + 1, 69)])      # keep = 211: inside chunk 3
    rows["median30"] = run_row([(30, 41), (31, 7), (200, 9), (100000, 2)])
    c = int(cut[3])                                                                   # median 3; the mode is the cut's own value (a tie
    rows["next_beyond_cut"] = run_row([(1, 10), (3, 9), (c, 10), (c + 1, 3)])         # with 1 goes up), mode + 1 is there but cut away
    return rows


def width_of(row):
    top = int(np.max(row))
    return 1 if top < 256 else 2 if top < 65536 else 4
