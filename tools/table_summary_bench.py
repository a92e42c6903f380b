"""--estimate-unknown's walks over the sample's counts on the device (SYLPH_HIP_UNKNOWN_DEVICE=1: five integers per sample from
csrc/table_summary.hip, nothing of the table copied to the host) against the parent commit, which copies every sample's k-mers and
counts into pageable vectors and walks the counts three times on the reporting thread (profiles/table_summary.txt).

Whole commands (the default): `sylph-hip profile -u` and `sylph-hip query -u` over --sketches (64) pre-sketched samples of --entries
entries each against tools/row_stats_bench.py's database and samples (20 genomes held whole, chance hits on every other; counts
uniform in 1..29, so the walk's state hovers near 15).  This tree's binary with SYLPH_HIP_UNKNOWN_DEVICE=1 alternates with the binary
of --parent (a directory that holds the parent commit's sylph-hip and its two libraries) on the same files, every command started
--settle seconds after the previous one exited; median of --reps runs with the spread (max - min); stdout must be byte-identical.
Without --parent the baseline is this tree's binary with SYLPH_HIP_UNKNOWN_DEVICE=0, and the file says so.  The road ships on by
default only if BOTH commands beat the baseline by more than the two spreads together.  One more, untimed run with
SYLPH_HIP_FEED_TRACE=1 gives the rung that answered per sample.

--kernels (a run apart): samples through a pipeline with the option "table_summary" and with want_table, through the binding — the
bytes copied per sample on each road and the "table_summary" family's time by the library's timers.  No share of peak is stated.

--headline DIR (a run apart): bench.py's headline on this tree and on a checkout of the parent commit in DIR (built), alternating.

GPU box: python tools/table_summary_bench.py [--parent DIR] [--out FILE];  ... --kernels;  ... --headline DIR"""
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
from row_stats_bench import make_table  # noqa: E402
from sylsp_profile_bench import make_database, write_sylsp  # noqa: E402

TRACE = re.compile(r"^\[sylph_hip feed\] unknown (\S+): road ([a-z ()]+), rung (\d+), (\d+) chunks walked again$", re.M)


def commands(a, emit):
    d = tempfile.mkdtemp(prefix="sylph_table_summary_bench_")
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
        emit(dict(what="sylph-hip profile -u / query -u over sketch files", sketches=a.sketches, entries_per_sketch=n_entries // a.sketches,
                  database_genomes=a.genomes, database_kmers=int(db_off[-1]), reps=a.reps, settle_seconds=a.settle,
                  baseline="the parent commit's binary" if a.parent else "this tree's binary with SYLPH_HIP_UNKNOWN_DEVICE=0"))

        def run(exe, cmd, unknown, trace=False):
            env = dict(os.environ, SYLPH_HIP_UNKNOWN_DEVICE=unknown)
            if trace:
                env["SYLPH_HIP_FEED_TRACE"] = "1"
            time.sleep(a.settle)
            t = time.perf_counter()
            p = subprocess.run([exe, cmd, db, "-u"] + files, capture_output=True, text=True, env=env, timeout=1800)
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
                print(f"# {cmd} -u rep {rep}: {new[-1]:.3f} s against {base[-1]:.3f} s", flush=True)
            assert same, f"{cmd} -u: stdout differs between the two binaries"
            med_n, med_b = float(np.median(new)), float(np.median(base))
            spread_n, spread_b = max(new) - min(new), max(base) - min(base)
            verdicts.append(bool(med_n + spread_n + spread_b < med_b))
            roads = TRACE.findall(run(new_exe, cmd, "1", trace=True)[2])
            emit(dict(command=cmd + " -u", device_seconds=[round(x, 3) for x in new], baseline_seconds=[round(x, 3) for x in base],
                      device_median=round(med_n, 3), device_spread=round(spread_n, 3), baseline_median=round(med_b, 3), baseline_spread=round(spread_b, 3),
                      device_ms_per_sketch=round(1e3 * med_n / a.sketches, 2), baseline_ms_per_sketch=round(1e3 * med_b / a.sketches, 2),
                      speedup=round(med_b / med_n, 3), stdout_byte_identical=same, beats_baseline_by_more_than_both_spreads=verdicts[-1],
                      samples_on_the_device_road=sum(1 for m in roads if m[1] == "device"), samples_declined=sum(1 for m in roads if m[1] != "device"),
                      rungs=sorted({int(m[2]) for m in roads}), chunks_walked_again=sum(int(m[3]) for m in roads),
                      output_lines=len(out_base.splitlines())))
        emit(dict(on_by_default=all(verdicts), rule="both commands beat the baseline by more than the two spreads together"))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def kernels(a, emit):
    import sylph_amd as S
    d = tempfile.mkdtemp(prefix="sylph_table_summary_bench_")
    try:
        rng = np.random.default_rng(1)
        db_kmers, db_off = make_database(f"{d}/db.syldb", a.genomes, 1)
        ctx = S.Context(0)
        db = S.Database(ctx, db_kmers, db_off.astype(np.uint64))
        tables = [make_table(rng, db_kmers, db_off, a.entries) for _ in range(4)]
        raws = [np.ascontiguousarray(t).view(np.uint8).reshape(-1) for t in tables]
        for road in ("host", "device"):
            p = S.Pipeline(db, c=200, paired=True, n_workers=2, depth=4, max_batch=1, want_table=road == "host")
            if road == "device":
                p.set_option("table_summary", "1")
            p.profile(True)
            per, t0 = [], time.perf_counter()
            for rep in range(a.reps + 1):
                for i, raw in enumerate(raws):
                    assert p.submit_entries(raw.ctypes.data, len(tables[i]), tag=i)
                for i in range(len(raws)):
                    r = p.next()
                    if road == "host":
                        per.append(dict(n_table=r["n_table"], bytes=r["n_table"] * 12))
                    else:
                        s = p.summary_of_last()
                        per.append(dict(n_table=r["n_table"], bytes=48, rung=s["rung"], open_chunks=s["open_chunks"], declined=s["flags"] & 1))
            wall = time.perf_counter() - t0
            ms, launches = p.kernel_stats("table_summary")
            rec = dict(what="one sample per probe batch through the pipeline", road=road, samples=per[:len(raws)],
                       table_bytes_copied_per_sample=float(np.median([x["bytes"] for x in per])), wall_ms_per_sample=round(1e3 * wall / len(per), 3))
            if road == "device":
                rec.update(table_summary_ms_per_sample=round(ms / max(1, launches), 4), table_summary_calls=int(launches),
                           note="family table_summary = the memset and every rung's three launches (HIP events around them)")
            emit(rec)
            p.close()
        db.close()
        ctx.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def headline(a, emit):
    trees = dict(this=ROOT, parent=os.path.abspath(a.headline))
    vals = dict(this=[], parent=[])
    for rep in range(a.reps):
        for name in (("this", "parent") if rep % 2 == 0 else ("parent", "this")):
            time.sleep(a.settle)
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--no-files-leg"],
                               cwd=trees[name], capture_output=True, text=True, timeout=1500)
            if p.returncode != 0:
                raise RuntimeError(p.stderr[-800:])
            vals[name].append(float(json.loads(p.stdout.strip().splitlines()[-1])["value"]))
            print(f"# bench.py on {name}: {vals[name][-1]:.1f}", flush=True)
    emit(dict(what="bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline --no-files-leg, alternating", this_tree=vals["this"], parent=vals["parent"],
              this_median=float(np.median(vals["this"])), parent_median=float(np.median(vals["parent"]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=64)
    ap.add_argument("--entries", type=int, default=1_900_000, help="entries per sketch (the table of a 1 Gbp pair at c = 200: about 1.9 M)")
    ap.add_argument("--genomes", type=int, default=20000, help="genomes of the synthetic database")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--settle", type=float, default=2.0)
    ap.add_argument("--parent", default="", help="directory with the parent commit's sylph-hip, libsylph_host.so and libsylph_hip.so")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--headline", default="", help="a built checkout of the parent commit: bench.py's headline on both trees")
    ap.add_argument("--out", default="", help="append the JSON lines to this file too")
    a = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    (kernels if a.kernels else headline if a.headline else commands)(a, emit)


if __name__ == "__main__":
    main()
