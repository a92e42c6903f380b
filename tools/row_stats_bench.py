"""The first pass's statistics head on the device (SYLPH_HIP_STATS_DEVICE=1: rows summarised by csrc/row_stats.hip, only the candidates
copied to the host) against the host's walk over every row with a hit (profiles/row_stats.txt).

Whole commands (the default): `sylph-hip profile` and `sylph-hip query` over --sketches (64) pre-sketched samples of --entries
entries each against a database of --genomes synth.decoy_sketches genomes (20,000 by default, written as a .syldb by
tools/sylsp_profile_bench.py's make_database); every sample holds the k-mers of 20 of the genomes whole and, beside them, k-mers
drawn from the whole database at random, so that every genome has a row of chance hits that fails the ANI cut.  This tree's binary
with SYLPH_HIP_STATS_DEVICE=1 alternates with the binary of --parent (a directory that holds the parent commit's sylph-hip and its
two libraries) on the same files, every command started --settle seconds after the previous one exited; median of --reps runs with the spread (max - min).  Without --parent the baseline is
this tree's binary with SYLPH_HIP_STATS_DEVICE=0, and the file says so.  The road ships on by default only if BOTH commands beat the
baseline by more than the two spreads together.  One more, untimed pair of runs with SYLPH_HIP_FEED_TRACE=1 gives the rows with
hits (host road) and the candidates (device road) per sample.

--kernels (a run apart): one sample through a pipeline with and without the row filter, through the binding — the bytes of result
copied per sample on each road and the "row_stats" family's time by the library's timers.  No share of peak is stated.

GPU box: python tools/row_stats_bench.py [--parent DIR] [--out FILE];  python tools/row_stats_bench.py --kernels [--out FILE]"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sylsp_profile_bench import ENTRY, make_database, write_sylsp  # noqa: E402

TRACE = re.compile(r"^\[sylph_hip feed\] stats (\S+): road (\w+), (?:(\d+) rows with hits, )?(\d+) candidates$", re.M)


def make_table(rng, db_kmers, db_off, n_entries):
    """A sample that holds 20 genomes of the database whole and, beside them, k-mers drawn from the whole database at random: every
    genome gets chance hits (n_entries / genomes of them on average) that fill a row and fail the ANI cut, as at GTDB scale."""
    G = len(db_off) - 1
    held = np.concatenate([db_kmers[db_off[g]:db_off[g + 1]] for g in rng.choice(G, size=min(G, 20), replace=False)])
    chance = db_kmers[rng.integers(0, len(db_kmers), size=max(0, n_entries - len(held)))]
    kmers = np.unique(np.concatenate([held, chance]))
    e = np.zeros(len(kmers), dtype=ENTRY)
    e["kmer"], e["count"] = kmers, rng.integers(1, 30, size=len(kmers))
    return e


def commands(a, emit):
    d = tempfile.mkdtemp(prefix="sylph_row_stats_bench_")
    try:
        rng = np.random.default_rng(1)
        db = f"{d}/db.syldb"
        db_kmers, db_off = make_database(db, a.genomes, 1)
        files, n_entries = [], 0
        for i in range(a.sketches):
            e = make_table(rng, db_kmers, db_off, a.entries)
            n_entries += len(e)
            files.append(f"{d}/sample_{i:03d}.sylsp")
            write_sylsp(files[-1], e, f"sample_{i:03d}.fq")
        new_exe = os.path.join(ROOT, "sylph_amd", "sylph-hip")
        base_exe = os.path.join(a.parent, "sylph-hip") if a.parent else new_exe
        emit(dict(what="sylph-hip profile / query over sketch files, default flags", sketches=a.sketches, entries_per_sketch=n_entries // a.sketches,
                  database_genomes=a.genomes, database_kmers=int(db_off[-1]), reps=a.reps, settle_seconds=a.settle,
                  baseline="the parent commit's binary" if a.parent else "this tree's binary with SYLPH_HIP_STATS_DEVICE=0"))

        def run(exe, cmd, stats, trace=False):
            env = dict(os.environ, SYLPH_HIP_STATS_DEVICE=stats)
            if trace:
                env["SYLPH_HIP_FEED_TRACE"] = "1"
            time.sleep(a.settle)
            t = time.perf_counter()
            p = subprocess.run([exe, cmd, db] + files, capture_output=True, text=True, env=env, timeout=1800)
            dt = time.perf_counter() - t
            if p.returncode != 0:
                raise RuntimeError(p.stderr[-800:])
            return dt, p.stdout, p.stderr

        run(new_exe, "profile", "1")                                         # untimed: binaries, libraries and the files come off the disk
        verdicts = []
        for cmd in ("profile", "query"):
            new, base, same = [], [], True
            for rep in range(a.reps):
                first_new = rep % 2 == 0                                     # which binary goes first alternates too
                if first_new:
                    dt, out_new, _ = run(new_exe, cmd, "1")
                dt_b, out_base, _ = run(base_exe, cmd, "0")
                if not first_new:
                    dt, out_new, _ = run(new_exe, cmd, "1")
                new.append(dt)
                base.append(dt_b)
                same = same and out_new == out_base
                print(f"# {cmd} rep {rep}: {new[-1]:.3f} s against {base[-1]:.3f} s", flush=True)
            med_n, med_b = float(np.median(new)), float(np.median(base))
            spread_n, spread_b = max(new) - min(new), max(base) - min(base)
            verdicts.append(bool(same and med_n + spread_n + spread_b < med_b))
            hits = [int(m[2]) for m in TRACE.findall(run(new_exe, cmd, "0", trace=True)[2]) if m[1] == "host"]
            cands = [int(m[3]) for m in TRACE.findall(run(new_exe, cmd, "1", trace=True)[2]) if m[1] == "device"]
            emit(dict(command=cmd, device_seconds=[round(x, 3) for x in new], baseline_seconds=[round(x, 3) for x in base],
                      device_median=round(med_n, 3), device_spread=round(spread_n, 3), baseline_median=round(med_b, 3), baseline_spread=round(spread_b, 3),
                      device_ms_per_sketch=round(1e3 * med_n / a.sketches, 2), baseline_ms_per_sketch=round(1e3 * med_b / a.sketches, 2),
                      speedup=round(med_b / med_n, 3), stdout_byte_identical=same, beats_baseline_by_more_than_both_spreads=verdicts[-1],
                      rows_with_hits_per_sample=dict(min=min(hits), median=float(np.median(hits)), max=max(hits)) if hits else None,
                      candidates_per_sample=dict(min=min(cands), median=float(np.median(cands)), max=max(cands)) if cands else None,
                      output_lines=len(out_base.splitlines())))
        emit(dict(on_by_default=all(verdicts), rule="both commands beat the baseline by more than the two spreads together"))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def kernels(a, emit):
    import ctypes as C

    import sylph_amd as S
    from sylph_amd import binding as B
    d = tempfile.mkdtemp(prefix="sylph_row_stats_bench_")
    try:
        rng = np.random.default_rng(1)
        db_kmers, db_off = make_database(f"{d}/db.syldb", a.genomes, 1)
        H = C.CDLL(os.path.join(ROOT, "sylph_amd", "libsylph_host.so"))
        ctx = S.Context(0)
        db = S.Database(ctx, db_kmers, db_off.astype(np.uint64))
        G = len(db_off) - 1
        tables = [make_table(rng, db_kmers, db_off, a.entries) for _ in range(4)]
        raws = [np.ascontiguousarray(t).view(np.uint8).reshape(-1) for t in tables]
        for cmd, pseudotax in (("profile", 1), ("query", 0)):
            filt = B.RowFilter()
            H.sylph_host_row_filter(C.c_uint64(31), C.c_double(3.0), C.c_double(-1.0), pseudotax, 0, C.byref(filt))
            for road in ("host", "device"):
                p = S.Pipeline(db, c=200, paired=True, n_workers=2, depth=4, max_batch=1)
                if road == "device":
                    p.set_row_filter(filt)
                p.profile(True)
                per = []
                for rep in range(a.reps + 1):
                    for i, raw in enumerate(raws):
                        assert p.submit_entries(raw.ctypes.data, len(tables[i]), tag=i)
                    for i in range(len(raws)):
                        r = p.next()
                        if road == "host":
                            per.append(dict(rows_with_hits=int((r["contain_count"] > 0).sum()), n_covs=r["n_covs"], width=r["cov_width"],
                                            bytes=(G + 1) * 8 + G * 4 + r["n_covs"] * r["cov_width"]))
                        else:
                            rows, off, covs = p.rows_of_last()
                            per.append(dict(candidates=len(rows), values=len(covs), width=r["cov_width"],
                                            bytes=len(rows) * 36 + (len(rows) + 1) * 8 + len(covs) * r["cov_width"] + 16))
                ms, launches = p.kernel_stats("row_stats")
                rec = dict(what="one sample per probe batch through the pipeline", filter_of=cmd, road=road, database_genomes=G, samples=per[:len(raws)],
                           result_bytes_per_sample_median=float(np.median([x["bytes"] for x in per])))
                if road == "device":
                    rec.update(row_stats_ms_per_launch=round(ms / max(1, launches), 4), row_stats_launches=int(launches),
                               note="family row_stats = both kernels, the two exclusive sums between them and the sample offsets (HIP events around the launches)")
                emit(rec)
                p.close()
        db.close()
        ctx.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=64)
    ap.add_argument("--entries", type=int, default=1_900_000, help="entries per sketch (the table of a 1 Gbp pair at c = 200: about 1.9 M)")
    ap.add_argument("--genomes", type=int, default=20000, help="genomes of the synthetic database")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--settle", type=float, default=2.0)
    ap.add_argument("--parent", default="", help="directory with the parent commit's sylph-hip, libsylph_host.so and libsylph_hip.so")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default="", help="append the JSON lines to this file too")
    a = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    (kernels if a.kernels else commands)(a, emit)


if __name__ == "__main__":
    main()
