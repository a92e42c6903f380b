#!/usr/bin/env python3
"""The bootstrap confidence intervals of one synthetic sample, host loop against device call (profiles/bootstrap_device.txt).
Input: 100 genomes, n_total lognormal around 16,500 k-mers, lambda in [0.1, 2], containment 0.2 - 0.9 — once (query) and twice (profile:
two get_stats passes).  Timed: the host loop of a libsylph_host.so (--parent-lib: the one built from the commit before the device
route, whose loop is the baseline) at 1, 3 and 16 threads, as stats(no_ci=0) - stats(no_ci=1); this tree's host loop the same way; the
device call with its copies (host clock around sylph_bootstrap_counts, which ends in a synchronise) and its kernels alone (hipEvent
pairs: sylph_ctx_kernel_stats "bootstrap"), for both kernel shapes; and `sylph-hip profile` as a whole with the route off and on.
Usage: python tools/bootstrap_bench.py [--parent-lib PATH] [--repeats 7] [--no-cli]"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sylph_amd as S                                    # noqa: E402
from sylph_amd import binding as B                       # noqa: E402
from tests.bootstrap_ref import HostStats                # noqa: E402


def sample(seed=2024, genomes=100):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(genomes):
        n = int(np.clip(rng.lognormal(np.log(16500), 0.5), 2000, 120000))
        lam, contain = rng.uniform(0.1, 2.0), rng.uniform(0.2, 0.9)
        covs = rng.poisson(lam, size=n)[rng.random(n) < contain]
        out.append((np.sort(covs[covs > 0]).astype(np.uint32), n))
    return out


def host_lib(path):
    L = C.CDLL(path)
    L.sylph_host_stats.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.POINTER(HostStats)]
    return L


def host_seconds(L, vectors, threads, no_ci):
    def one(v):
        out = HostStats()
        L.sylph_host_stats(v[0].ctypes.data_as(C.c_void_p), len(v[0]), v[1], 31, 3.0, 0.0, 0, no_ci, 0, 0, C.byref(out))
        return out.has_ci
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as pool:           # (ctypes releases the interpreter lock during the call)
        n_ci = sum(pool.map(one, vectors))
    return time.perf_counter() - t0, n_ci


def spread(xs):
    return f"median {statistics.median(xs) * 1e3:9.3f} ms   min {min(xs) * 1e3:9.3f}   max {max(xs) * 1e3:9.3f}   (n = {len(xs)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-cli", action="store_true")
    a = ap.parse_args()
    base = sample()
    print(f"input: {len(base)} genomes, {sum(n for _, n in base)} k-mers, {sum(len(c) for c, _ in base)} hits; x1 = query, x2 = profile")
    ctx = S.Context(0)
    # (this tree's libraries first: a parent library loaded behind them binds to this tree's libsylph_hip.so, a superset of its own)
    loaded = [("this tree", host_lib(os.path.join(ROOT, "sylph_amd", "libsylph_host.so")))]
    if a.parent_lib:
        loaded.append(("parent commit", host_lib(os.path.abspath(a.parent_lib))))
    medians = {}
    for passes in (1, 2):
        vectors = base * passes
        print(f"\n== {passes} pass(es): {len(vectors)} statistics, {sum(n for _, n in vectors) * 100} draws")
        for name, L in loaded:
            for threads in (1, 3, 16):
                host_seconds(L, vectors, threads, 0)                 # warm-up
                with_ci, without = [], []
                for _ in range(a.repeats if threads > 1 else max(3, a.repeats // 2)):
                    t1, n_ci = host_seconds(L, vectors, threads, 0)
                    t0, _ = host_seconds(L, vectors, threads, 1)
                    with_ci.append(t1)
                    without.append(t0)
                loop = [x - y for x, y in zip(with_ci, without)]
                medians[(name, passes, threads)] = (statistics.median(loop), min(loop), max(loop))
                print(f"host loop, {name:13s} {threads:2d} threads: {spread(loop)}   [statistics without CI: {statistics.median(without) * 1e3:.3f} ms; {n_ci} intervals]")
        # the device call: the genomes that want an interval, as report() hands them over (kept prefix = whole row here)
        items = [v for v in vectors if len(v[0]) >= 25]
        covs = np.concatenate([c for c, _ in items])
        width = np.uint8 if covs.max() < 256 else np.uint16
        covs = covs.astype(width)
        off = np.zeros(len(items) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(c) for c, _ in items])
        keep = np.array([len(c) for c, _ in items], dtype=np.uint32)
        n_total = np.array([n for _, n in items], dtype=np.uint32)
        results = {}
        for shape in ("gather", "table"):
            ctx.set_option("bootstrap_shape", shape)
            for _ in range(3):
                results[shape] = B.bootstrap_counts(ctx, covs, off, keep, n_total)
            wall = []
            for _ in range(a.repeats * 3):
                t0 = time.perf_counter()
                B.bootstrap_counts(ctx, covs, off, keep, n_total)
                wall.append(time.perf_counter() - t0)
            ctx.profile(True)
            kern = []
            for _ in range(a.repeats * 3):
                before = ctx.kernel_stats("bootstrap")[0]
                B.bootstrap_counts(ctx, covs, off, keep, n_total)
                ctx.synchronize()
                kern.append((ctx.kernel_stats("bootstrap")[0] - before) * 1e-3)
            ctx.profile(False)
            medians[(shape, passes)] = (statistics.median(wall), min(wall), max(wall))
            print(f"device call, {shape:6s} with copies : {spread(wall)}   [{len(items)} items, {covs.nbytes} bytes up, {len(items) * 2000} bytes down]")
            print(f"device call, {shape:6s} kernels only: {spread(kern)}")
        assert np.array_equal(results["gather"][0], results["table"][0]) and not results["gather"][1].any()
        ctx.set_option("bootstrap_shape", "gather")
    if a.parent_lib:
        print("\n== the bar: device call with copies (default shape) against the parent's host loop at 16 threads")
        for passes in (1, 2):
            h, d = medians[("parent commit", passes, 16)], medians[("gather", passes)]
            print(f"{passes} pass(es): host {h[0] * 1e3:.3f} ms [{h[1] * 1e3:.3f}, {h[2] * 1e3:.3f}]   device {d[0] * 1e3:.3f} ms [{d[1] * 1e3:.3f}, {d[2] * 1e3:.3f}]"
                  f"   -> {'device faster beyond both spreads' if d[2] < h[1] else 'NOT separated'}")
    ctx.close()
    if a.no_cli:
        return
    from tests.test_gpu_cli_bootstrap import BIN, build_inputs
    with tempfile.TemporaryDirectory() as tmp:
        d = build_inputs(Path(tmp), os.path.join(ROOT, "tests", "golden"))
        print("\n== sylph-hip profile, golden E. coli inputs (thinned reads: the genomes get intervals), whole command, median of 3, 2 s apart")
        for route in ("0", "1", "0", "1"):
            ts = []
            for _ in range(3):
                time.sleep(2)
                env = dict(os.environ, SYLPH_HIP_BOOTSTRAP_DEVICE=route, SYLPH_HIP_EXACT_DEDUP="1")
                t0 = time.perf_counter()
                p = subprocess.run([BIN, "profile", str(d["db"]), "-c", "50", "-1", str(d["dir"] / "thin_1.fq"), "-2", str(d["dir"] / "thin_2.fq")],
                                   capture_output=True, text=True, env=env, timeout=300)
                ts.append(time.perf_counter() - t0)
                assert p.returncode == 0, p.stderr[-2000:]
            print(f"SYLPH_HIP_BOOTSTRAP_DEVICE={route}: median {statistics.median(ts):.3f} s   {['%.3f' % t for t in ts]}   rows {len(p.stdout.splitlines()) - 1}")


if __name__ == "__main__":
    main()
