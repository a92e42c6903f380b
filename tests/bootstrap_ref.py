"""What the bootstrap tests share (tests/test_bootstrap_plan.py, tests/test_gpu_bootstrap.py, tests/golden/make_bootstrap_ci.py): a
sequential WyRand + Lemire in Python ints (fastrand 2.1.1's published definition), a numpy restatement of the position-addressed draws
with its 128-bit products made from 32-bit halves, the summary ratio_lambda / ani_from_lambda read off a resample, and the coverage
vectors the host-level tests run.  Nothing here calls the code under test."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

WY_ADD, WY_XOR, M64 = 0x2D358DCCAA6C78A5, 0x8BB84B93962EACC9, (1 << 64) - 1
BINS = 64
SUMMARY_FIELDS = ("n_nonzero", "n_distinct", "mode", "mode_count", "next_count")


class HostStats(C.Structure):            # SylphHostStats, sylph_amd/host/capi.cpp
    _fields_ = [(n, C.c_double) for n in ("naive_ani", "final_est_ani", "final_est_cov", "mean_cov", "median_cov", "lambda_",
                                          "ani_ci_lo", "ani_ci_hi", "lambda_ci_lo", "lambda_ci_hi")] + \
               [("lambda_status", C.c_int32), ("passed", C.c_int32), ("has_ci", C.c_int32), ("pad", C.c_int32),
                ("contain_count", C.c_uint64), ("n_kmers", C.c_uint64)]


CI_FIELDS = ("ani_ci_lo", "ani_ci_hi", "lambda_ci_lo", "lambda_ci_hi")


class SequentialWyRand:
    """fastrand's generator, one call after the other: next() steps the state, below(n) is Lemire's bounded integer WITH its rejection
    loop; .rejections lists the positions (0-based next() calls) whose output was rejected."""

    def __init__(self, seed):
        self.s, self.calls, self.rejections = seed, 0, []

    def next(self):
        self.s = (self.s + WY_ADD) & M64
        t = self.s * (self.s ^ WY_XOR)
        self.calls += 1
        return (t & M64) ^ (t >> 64)

    def below(self, n):
        m = self.next() * n
        hi, lo = m >> 64, m & M64
        if lo < n:
            t = ((1 << 64) - n) % n
            while lo < t:
                self.rejections.append(self.calls - 1)
                m = self.next() * n
                hi, lo = m >> 64, m & M64
        return hi


def _mul_64x64(a, b):
    """(lo, hi) of a * b for uint64 arrays, from 32-bit halves (no partial sum overflows 64 bits)"""
    m32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    a0, a1, b0, b1 = a & m32, a >> s32, b & m32, b >> s32
    p00 = a0 * b0
    p01 = a0 * b1 + (p00 >> s32)
    p10 = a1 * b0 + (p01 & m32)
    hi = a1 * b1 + (p01 >> s32) + (p10 >> s32)
    lo = (p10 << s32) | (p00 & m32)
    return lo, hi


def draws(seed, first, count, n):
    """Draws first .. first + count - 1 of the stream seeded with `seed`, as indices below n, assuming no rejection anywhere — and asserts
    that none of THESE draws would have been rejected."""
    with np.errstate(over="ignore"):
        j = np.arange(first + 1, first + count + 1, dtype=np.uint64)
        state = np.uint64(seed) + j * np.uint64(WY_ADD)
        lo, hi = _mul_64x64(state, state ^ np.uint64(WY_XOR))
        r = lo ^ hi
        if n < (1 << 32):                                                     # r * n in 96 bits: two products
            m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
            a = (r & m32) * np.uint64(n)
            b = (r >> s32) * np.uint64(n) + (a >> s32)
            lo, hi = (b << s32) | (a & m32), b >> s32
        else:
            lo, hi = _mul_64x64(r, np.full(count, n, dtype=np.uint64))
    thr = ((1 << 64) - n) % n
    assert not (lo < np.uint64(thr)).any(), "the reference met a rejected draw"
    return hi


def summary_of_values(values):
    """(n_nonzero, n_distinct saturating at 2, mode with ties to the larger value, mode_count, count of mode + 1): ratio_lambda's reading
    (inference.rs:207-242) of a vector of coverage values"""
    v = np.asarray(values)
    v = v[v != 0]
    if len(v) == 0:
        return (0, 0, 0, 0, 0)
    vals, cnt = np.unique(v, return_counts=True)
    best = sorted(zip(cnt.tolist(), vals.tolist()), reverse=True)[0]          # sort (count, value) descending, take the first
    mode_count, mode = best
    nxt = cnt[vals == mode + 1]
    return (int(len(v)), min(2, len(vals)), int(mode), int(mode_count), int(nxt[0]) if len(nxt) else 0)


def resample_summaries(kept, n_total, seed, iters):
    """The summaries of `iters` resamples of full_covs = n_total - len(kept) zeros + kept, drawn from one stream seeded with `seed`"""
    kept = np.asarray(kept, dtype=np.int64)
    n_zero = n_total - len(kept)

    def one(it):
        idx = draws(seed, it * n_total, n_total, n_total).astype(np.int64)
        nz = idx[idx >= n_zero] - n_zero
        c = np.bincount(kept[nz], minlength=2) if len(nz) else np.zeros(2, dtype=np.int64)
        c[0] = 0
        n_nonzero, distinct = int(c.sum()), int((c > 0).sum())
        if n_nonzero == 0:
            return (0, 0, 0, 0, 0)
        top = int(c.max())
        mode = int(np.nonzero(c == top)[0][-1])                               # ties: the larger value
        return (n_nonzero, min(2, distinct), mode, top, int(c[mode + 1]) if mode + 1 < len(c) else 0)

    if n_total * iters < (1 << 22):
        return [one(it) for it in range(iters)]
    with ThreadPoolExecutor(max_workers=8) as pool:                           # (numpy releases the interpreter lock: 10^8 draws in seconds)
        return list(pool.map(one, range(iters)))


def oracle_shaped_vectors():
    """(covs, n_kmers) of tests/test_host.py::test_stats_match_oracle's 300 trials, then test_bootstrap_ci_is_deterministic_and_ordered's"""
    rng = np.random.default_rng(0)
    out = []
    for trial in range(300):
        n_kmers = int(rng.integers(50, 30000))
        lam = float(rng.choice([0.02, 0.1, 0.5, 1.0, 2.5, 8.0, 40.0]))
        hit = rng.random(n_kmers) < rng.uniform(0.05, 1.0)
        covs = rng.poisson(lam, size=n_kmers)[hit]
        covs = covs[covs > 0].astype(np.uint32)
        if trial % 7 == 0 and len(covs):
            covs[rng.integers(0, len(covs), size=3)] = 100000
        out.append((covs, n_kmers))
    rng = np.random.default_rng(3)
    covs = rng.poisson(0.8, size=5000)
    out.append((covs[covs > 0].astype(np.uint32), 8000))
    return out


def host_level_vectors():
    """60 Poisson vectors (lambda in {0.05, 0.3, 1, 2.5}, hit rate 0.2 - 1) and three special ones: all values equal, fewer than 25
    non-zero, three outliers above the Poisson cap"""
    rng = np.random.default_rng(11)
    out = []
    for i in range(60):
        n_kmers = int(rng.integers(300, 6000))
        lam = (0.05, 0.3, 1.0, 2.5)[i % 4]
        hit = rng.random(n_kmers) < rng.uniform(0.2, 1.0)
        covs = rng.poisson(lam, size=n_kmers)[hit]
        out.append((covs[covs > 0].astype(np.uint32), n_kmers))
    out.append((np.full(900, 2, dtype=np.uint32), 1500))
    out.append((np.array([1] * 12 + [2] * 7, dtype=np.uint32), 400))
    covs = rng.poisson(1.0, size=3000)
    covs = covs[covs > 0].astype(np.uint32)
    covs[[5, 50, 500]] = 100000
    out.append((covs, 3500))
    return out
