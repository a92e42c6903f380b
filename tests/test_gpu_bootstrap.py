"""GPU tests of the bootstrap on the device (sylph_bootstrap_counts, sylph_amd/csrc/bootstrap.hip): every count of every resample
against tests/bootstrap_ref.py's numpy restatement (which asserts that it met no rejected draw), for both ways from a drawn index to its
value; items that decline, invalid arguments, the grid's extremes; and, through the host's batch entry (sylph_host_stats_batch), the
confidence intervals of `profile` / `query` bit for bit against the host's own loop."""
import ctypes as C
import os

import numpy as np
import pytest

import sylph_amd as S
from sylph_amd import binding as B

from . import bootstrap_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_TOTALS = (1, 25, 26, 63, 64, 65, 255, 256, 257, 1000, 20011, 65537)
SEEDS = (7, 0x9E3779B97F4A7C15)


def as_tuples(rows):
    return [tuple(int(r[f]) for f in R.SUMMARY_FIELDS) for r in rows]


@pytest.fixture(scope="module")
def items():
    """One call's worth of items: every n_total with keep = 0, 1, all, about a third; rows longer than `keep` (gaps), values 1 .. 63"""
    rng = np.random.default_rng(42)
    rows, keep, n_total = [], [], []
    for n in N_TOTALS:
        for k in sorted({0, 1, n, max(1, n // 3)}):
            vals = np.sort(np.minimum(1 + rng.poisson(rng.choice([0.3, 1.0, 4.0]), size=k + int(rng.integers(0, 9))), R.BINS - 1))
            rows.append(vals.astype(np.uint32))
            keep.append(k)
            n_total.append(n)
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return dict(rows=rows, covs=np.concatenate(rows), off=off, keep=np.array(keep, dtype=np.uint32), n_total=np.array(n_total, dtype=np.uint32))


@pytest.fixture(scope="module")
def expected(items):
    """seed -> per item the 100 resamples' summaries (computed once; resample 0 is also what iters = 1 must give)"""
    return {seed: [R.resample_summaries(row[:k], int(n), seed, 100) for row, k, n in zip(items["rows"], items["keep"], items["n_total"])]
            for seed in SEEDS}


@pytest.mark.parametrize("shape", ["gather", "table"])
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32])
def test_counts_equal_the_restatement(ctx, items, expected, dtype, mem, shape):
    import torch
    ctx.set_option("bootstrap_shape", shape)
    try:
        covs = items["covs"].astype(dtype)
        dev = torch.from_numpy(covs.view(np.uint8).copy()).cuda() if mem == "device" else None
        torch.cuda.synchronize()
        for seed, iters in ((SEEDS[0], 1), (SEEDS[0], 100), (SEEDS[1], 100)):
            if mem == "device":
                out, declined = B.bootstrap_counts(ctx, dev.data_ptr(), items["off"], items["keep"], items["n_total"], seed=seed, iters=iters,
                                                   cov_width=covs.dtype.itemsize)
            else:
                out, declined = B.bootstrap_counts(ctx, covs, items["off"], items["keep"], items["n_total"], seed=seed, iters=iters)
            assert not declined.any()
            for i, want in enumerate(expected[seed]):
                assert as_tuples(out[i]) == want[:iters], (seed, iters, i, int(items["n_total"][i]), int(items["keep"][i]))
    finally:
        ctx.set_option("bootstrap_shape", "gather")


@pytest.mark.parametrize("shape", ["gather", "table"])
def test_an_item_beyond_the_bins_declines_alone(ctx, items, expected, shape):
    ctx.set_option("bootstrap_shape", shape)
    try:
        rng = np.random.default_rng(1)
        base = np.sort(1 + rng.poisson(1.0, size=300)).astype(np.uint32)
        fits, beyond = base.copy(), base.copy()
        fits[-1], beyond[-1] = R.BINS - 1, R.BINS
        first = [i for i, n in enumerate(items["n_total"]) if n == 1000]          # a few ordinary items around the two
        rows = [items["rows"][first[0]], fits, items["rows"][first[1]], beyond, items["rows"][first[2]]]
        keep = np.array([items["keep"][first[0]], 300, items["keep"][first[1]], 300, items["keep"][first[2]]], dtype=np.uint32)
        n_total = np.array([1000, 700, 1000, 700, 1000], dtype=np.uint32)
        off = np.zeros(6, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in rows])
        out, declined = B.bootstrap_counts(ctx, np.concatenate(rows).astype(np.uint8), off, keep, n_total, seed=7, iters=100)
        assert declined.tolist() == [0, 0, 0, 1, 0]
        assert as_tuples(out[1]) == R.resample_summaries(fits, 700, 7, 100)
        for at, i in ((0, first[0]), (2, first[1]), (4, first[2])):
            assert as_tuples(out[at]) == expected[7][i]
    finally:
        ctx.set_option("bootstrap_shape", "gather")


def test_invalid_arguments_are_errors_and_the_context_lives_on(ctx, items, expected):
    covs = np.array([1, 1, 2, 3], dtype=np.uint32)
    ok = dict(cov_off=[0, 4], keep=[3], n_total=[10])
    bad = [dict(ok, keep=[11]),                    # keep > n_total
           dict(ok, keep=[5], n_total=[20]),       # keep > the row
           dict(ok, n_total=[0], keep=[0]),        # nothing to draw from
           dict(ok, iters=0)]
    for kw in bad:
        with pytest.raises(S.SylphHipError) as e:
            B.bootstrap_counts(ctx, covs, **kw)
        assert e.value.code == -1, kw
    L = S.load()
    one, flag = np.zeros(1, dtype=B.BOOTSTRAP_SUMMARY), np.zeros(1, dtype=np.uint8)
    args = [np.array(v, dtype=t) for v, t in (([0, 4], np.uint64), ([3], np.uint32), ([10], np.uint32))]
    call = lambda width: L.sylph_bootstrap_counts(ctx._h, covs.ctypes.data, width, *[a.ctypes.data for a in args], 1, B.MEM_HOST, 7, 1,
                                                   one.ctypes.data, flag.ctypes.data)
    assert call(3) == -1 and call(8) == -1 and call(0) == -1
    out, declined = B.bootstrap_counts(ctx, covs, [0], [], [])                    # no items: fine
    assert out.shape == (0, 100) and len(declined) == 0
    out, declined = B.bootstrap_counts(ctx, covs, **ok)
    assert not declined.any() and as_tuples(out[0]) == R.resample_summaries(covs[:3], 10, 7, 100)


def test_grid_extremes(ctx):
    # 65,536 items of one draw each: the draw is index 0 whatever the generator says, the value the item's only one (or a zero)
    n = 65536
    keep = (np.arange(n) % 2).astype(np.uint32)
    covs = (1 + np.arange(n) % 5).astype(np.uint8)
    out, declined = B.bootstrap_counts(ctx, covs, np.arange(n + 1, dtype=np.uint64), keep, np.ones(n, dtype=np.uint32), iters=100)
    assert not declined.any()
    want = np.zeros((n, 100), dtype=B.BOOTSTRAP_SUMMARY)
    k1 = keep == 1
    want["n_nonzero"][k1], want["n_distinct"][k1], want["mode_count"][k1] = 1, 1, 1
    want["mode"][k1] = covs[k1, None]
    assert np.array_equal(out, want)
    # one item of 2^20 draws x 100 resamples
    rng = np.random.default_rng(9)
    kept = np.sort(1 + rng.poisson(1.0, size=2**19)).astype(np.uint8)
    out, declined = B.bootstrap_counts(ctx, kept, [0, len(kept)], [len(kept)], [2**20], iters=100)
    assert not declined.any() and as_tuples(out[0]) == R.resample_summaries(kept, 2**20, 7, 100)


@pytest.fixture(scope="module")
def host():
    L = C.CDLL(os.path.join(ROOT, "sylph_amd", "libsylph_host.so"))
    L.sylph_host_stats.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.POINTER(R.HostStats)]
    L.sylph_host_stats_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_int,
                                         C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
    return L


def stats_batch(host, ctx, vectors, route, no_ci=0):
    off = np.zeros(len(vectors) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(v) for v, _ in vectors])
    covs = np.concatenate([v for v, _ in vectors]).astype(np.uint32)
    n_kmers = np.array([n for _, n in vectors], dtype=np.uint64)
    out, on_host = (R.HostStats * len(vectors))(), C.c_uint64(99)
    rc = host.sylph_host_stats_batch(ctx._h, covs.ctypes.data, off.ctypes.data, n_kmers.ctypes.data, len(vectors), 31, 3.0, 0.0, 0, no_ci, 0, 0, route,
                                     C.byref(out), C.byref(on_host))
    return rc, out, on_host.value


def test_device_route_gives_the_hosts_intervals_bit_for_bit(host, ctx):
    vectors = R.host_level_vectors()
    assert len(vectors) == 63
    rc, got, on_host = stats_batch(host, ctx, vectors, route=2)                   # device only: a declined item would be an error
    assert rc == 0 and on_host == 0
    with_ci = 0
    for i, (covs, n_kmers) in enumerate(vectors):
        cv, want = np.ascontiguousarray(covs, dtype=np.uint32), R.HostStats()
        host.sylph_host_stats(cv.ctypes.data_as(C.c_void_p), len(cv), n_kmers, 31, 3.0, 0.0, 0, 0, 0, 0, C.byref(want))
        assert bytes(got[i]) == bytes(want), i                                    # every field, the four CI doubles and has_ci among them
        with_ci += want.has_ci
    assert with_ci >= 20
    assert got[60].has_ci == 0 and got[61].has_ci == 0 and got[62].lambda_status == 2      # all equal / under 25 values: no lambda; outliers dropped
    # the host route and --no-ci through the same entry
    rc, again, on_host = stats_batch(host, ctx, vectors, route=0)
    assert rc == 0 and on_host == with_ci_items(got) and all(bytes(a) == bytes(b) for a, b in zip(again, got))
    rc, none, on_host = stats_batch(host, ctx, vectors, route=2, no_ci=1)
    assert rc == 0 and on_host == 0 and not any(s.has_ci for s in none)


def with_ci_items(stats):
    """items whose interval was resampled at all: a lambda was estimated (has_ci says whether 50 resamples gave one)"""
    return sum(1 for s in stats if s.passed and s.lambda_status == 2)


def test_a_declined_item_runs_the_hosts_loop_or_is_an_error_under_only(host, ctx):
    """No real call declines for its values (the Poisson cut-off of a median of at most 2 keeps them far below 64) and none of seconds
    for a rejected draw: the context's test knob "bootstrap_bins" lowers the bins so that ordinary genomes decline."""
    vectors = R.host_level_vectors()[:12]
    rc, want, on_host = stats_batch(host, ctx, vectors, route=0)
    assert rc == 0 and on_host == with_ci_items(want) >= 6
    ctx.set_option("bootstrap_bins", "2")                                         # every item that keeps a value above 1 declines
    try:
        rc, got, on_host = stats_batch(host, ctx, vectors, route=1)
        assert rc == 0 and on_host == with_ci_items(want) and all(bytes(a) == bytes(b) for a, b in zip(got, want))
        rc, _, _ = stats_batch(host, ctx, vectors, route=2)
        assert rc == -1
    finally:
        ctx.set_option("bootstrap_bins", "64")
    rc, got, on_host = stats_batch(host, ctx, vectors, route=2)
    assert rc == 0 and on_host == 0 and all(bytes(a) == bytes(b) for a, b in zip(got, want))
