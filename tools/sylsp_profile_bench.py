"""Pre-sketched samples through `sylph-hip profile`: the device's road (tables unpacked on the GPU, samples through the pipeline)
against the host's (profiles/sylsp_pipeline.txt).

Whole commands (the default): `sylph-hip profile db.syldb *.sylsp`, default flags, over --sketches (64) sketch files whose tables
have --entries (1.9 M: the table of bench.py's 1 Gbp pair) entries each, in two sets: `ascending` (as write_sylsp writes them) and
`shuffled` (the same tables in random entry order, standing in for the reference's hashbrown order).  The database is
synth.decoy_sketches' — bench.py's generator of sketch-only genomes — written as a .syldb; every sample holds the k-mers of 20 of
its genomes and random ones beside them.  This tree's binary with SYLPH_HIP_SYLSP_DEVICE=1 alternates with the binary of --parent (a
directory that holds the parent commit's sylph-hip and its two libraries, which knows the host's road only) on the same files, every
command started --settle seconds after the previous one exited; median of --reps runs with the spread (max - min).  Without
--parent the baseline is this tree's binary with SYLPH_HIP_SYLSP_DEVICE=0, and the file says so.  The road ships on by default
only if BOTH sets beat the baseline by more than the two spreads together.

--kernels (a run apart): the unpack (family "sylsp") and the general road (families "sort" and "sylsp_dedup") by the library's
timers, through the binding, on entries already in device memory, with the bytes each moves per entry.  No share of peak is stated.

GPU box: python tools/sylsp_profile_bench.py [--parent DIR] [--out FILE];  python tools/sylsp_profile_bench.py --kernels [--out FILE]"""
import argparse
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENTRY = np.dtype([("kmer", "<u8"), ("count", "<u4")])


def bincode_str(s):
    return struct.pack("<Q", len(s)) + s


def make_database(path, n_genomes, seed):
    """synth.decoy_sketches as a .syldb (types.rs:163-173 as Vec<GenomeSketch>; an empty tracked list: `profile` asks for one)"""
    import synth
    kmers, off = synth.decoy_sketches(n_genomes, c=200, device="cuda", seed=seed)
    kmers, off = kmers.cpu().numpy().view(np.uint64), off.cpu().numpy().astype(np.int64)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", n_genomes))
        for g in range(n_genomes):
            mine = kmers[off[g]:off[g + 1]]
            f.write(struct.pack("<Q", len(mine)) + mine.tobytes() + b"\x01" + struct.pack("<Q", 0))
            f.write(bincode_str(f"decoy_{g}.fa".encode()) + bincode_str(f"decoy_{g}_contig".encode()))
            f.write(struct.pack("<QQQQ", 200, 31, int(len(mine) * 200 / 0.87), 30))
    return kmers, off


def make_table(rng, db_kmers, db_off, n_entries):
    G = len(db_off) - 1
    held = np.concatenate([db_kmers[db_off[g]:db_off[g + 1]] for g in rng.choice(G, size=min(G, 20), replace=False)])
    thr = (2**64 - 1) // 200                                                  # FracMinHash at c = 200 keeps the hashes below this
    kmers = np.unique(np.concatenate([held, rng.integers(0, thr, size=max(0, n_entries - len(held)), dtype=np.uint64)]))
    e = np.zeros(len(kmers), dtype=ENTRY)
    e["kmer"], e["count"] = kmers, rng.integers(1, 30, size=len(kmers))
    return e


def write_sylsp(path, entries, name):
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(entries)) + entries.tobytes() + struct.pack("<QQ", 200, 31) + bincode_str(name.encode()) + b"\x00\x01" + struct.pack("<d", 150.0))


def commands(a, emit):
    d = tempfile.mkdtemp(prefix="sylph_sylsp_bench_")
    try:
        rng = np.random.default_rng(1)
        db = f"{d}/db.syldb"
        db_kmers, db_off = make_database(db, a.genomes, 1)
        sets = {"ascending": [], "shuffled": []}
        n_entries = 0
        for i in range(a.sketches):
            e = make_table(rng, db_kmers, db_off, a.entries)
            n_entries += len(e)
            for kind in sets:
                sets[kind].append(f"{d}/{kind}_{i:03d}.sylsp")
                write_sylsp(sets[kind][-1], e if kind == "ascending" else e[rng.permutation(len(e))], f"sample_{i:03d}.fq")
        new_exe = os.path.join(ROOT, "sylph_amd", "sylph-hip")
        base_exe = os.path.join(a.parent, "sylph-hip") if a.parent else new_exe
        emit(dict(what="sylph-hip profile over sketch files, default flags", sketches=a.sketches, entries_per_sketch=n_entries // a.sketches,
                  sketch_bytes=os.path.getsize(sets["ascending"][0]), database_genomes=a.genomes, database_kmers=int(db_off[-1]), reps=a.reps,
                  settle_seconds=a.settle,
                  baseline="the parent commit's binary (host road)" if a.parent else "this tree's binary with SYLPH_HIP_SYLSP_DEVICE=0 (host road)"))

        def run(exe, kind, device, n_files=None):
            env = dict(os.environ, SYLPH_HIP_SYLSP_DEVICE=device, SYLPH_HIP_FEED_TRACE="1")
            time.sleep(a.settle)
            t = time.perf_counter()
            p = subprocess.run([exe, "profile", db] + sets[kind][:n_files], capture_output=True, text=True, env=env, timeout=1800)
            dt = time.perf_counter() - t
            if p.returncode != 0:
                raise RuntimeError(p.stderr[-800:])
            routes = {l.split(": route ")[1].split(",")[0] + ", " + l.split(", table ")[1].split(",")[0] for l in p.stderr.split("\n") if l.startswith("[sylph_hip feed] sylsp ")}
            return dt, routes, p.stdout

        run(new_exe, "ascending", "1")                                       # untimed: binaries, libraries and the files come off the disk
        verdicts, medians = [], {}
        for kind in sets:
            new, base, routes, same = [], [], set(), True
            for rep in range(a.reps):
                first_new = rep % 2 == 0                                     # which binary goes first alternates too
                if first_new:
                    dt, r, out_new = run(new_exe, kind, "1")
                dt_b, r_b, out_base = run(base_exe, kind, "0")
                if not first_new:
                    dt, r, out_new = run(new_exe, kind, "1")
                new.append(dt)
                base.append(dt_b)
                routes |= r
                same = same and out_new == out_base
                print(f"# {kind} rep {rep}: {new[-1]:.3f} s against {base[-1]:.3f} s", flush=True)
            med_n, med_b = float(np.median(new)), float(np.median(base))
            spread_n, spread_b = max(new) - min(new), max(base) - min(base)
            verdicts.append(bool(same and med_n + spread_n + spread_b < med_b))
            medians[kind] = (med_n, med_b)
            emit(dict(set=kind, routes=sorted(routes), device_seconds=[round(x, 3) for x in new], baseline_seconds=[round(x, 3) for x in base],
                      device_median=round(med_n, 3), device_spread=round(spread_n, 3), baseline_median=round(med_b, 3), baseline_spread=round(spread_b, 3),
                      device_ms_per_sketch=round(1e3 * med_n / a.sketches, 2), baseline_ms_per_sketch=round(1e3 * med_b / a.sketches, 2),
                      speedup=round(med_b / med_n, 2), stdout_byte_identical=same, beats_baseline_by_more_than_both_spreads=verdicts[-1]))
        emit(dict(on_by_default=all(verdicts), rule="both sets beat the baseline by more than the two spreads together"))
        if a.sketches > 1:
            # what a command costs before and beside its samples (process and runtime start, database load and index): the same command
            # over ONE sketch; what one more sketch costs: the difference to the full list, per sketch
            for kind in sets:
                one_n = float(np.median([run(new_exe, kind, "1", 1)[0] for _ in range(a.reps)]))
                one_b = float(np.median([run(base_exe, kind, "0", 1)[0] for _ in range(a.reps)]))
                med_n, med_b = medians[kind]
                emit(dict(set=kind, what="the command over one sketch, and the cost of one more sketch = (all - one) / (sketches - 1)",
                          device_one_sketch_seconds=round(one_n, 3), baseline_one_sketch_seconds=round(one_b, 3),
                          device_ms_per_further_sketch=round(1e3 * (med_n - one_n) / (a.sketches - 1), 2),
                          baseline_ms_per_further_sketch=round(1e3 * (med_b - one_b) / (a.sketches - 1), 2)))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def kernels(a, emit):
    import torch

    import sylph_amd as S
    from sylph_amd.binding import MEM_DEVICE
    rng = np.random.default_rng(2)
    kmers = np.unique(rng.integers(0, 2**63, size=a.entries, dtype=np.uint64))
    e = np.zeros(len(kmers), dtype=ENTRY)
    e["kmer"], e["count"] = kmers, rng.integers(1, 30, size=len(kmers))
    n = len(e)
    ctx = S.Context(0)
    ctx.profile(True)
    fams = ("sylsp", "sort", "sylsp_dedup")
    for kind, entries in (("ascending", e), ("shuffled", e[rng.permutation(n)])):
        raw = np.concatenate([np.zeros(16, np.uint8), entries.view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])
        dev = torch.from_numpy(raw).cuda()
        torch.cuda.synchronize()
        ms = {f: [] for f in fams}
        for rep in range(a.reps + 1):                                        # (the first repetition pays for the allocations: not counted)
            before = {f: ctx.kernel_stats(f)[0] for f in fams}
            t = S.Table(ctx, dev.data_ptr() + 16, n_entries=n, mem=MEM_DEVICE)
            assert t.was_ascending == (kind == "ascending") and t.n == n
            t.close()
            if rep:
                for f in fams:
                    ms[f].append(ctx.kernel_stats(f)[0] - before[f])
        med = {f: float(np.median(ms[f])) for f in fams}
        rec = dict(what="kernel times by the library's timers (HIP events around the launches), entries in device memory", set=kind, entries=n, reps=a.reps,
                   unpack_ms=[round(x, 4) for x in ms["sylsp"]], unpack_ms_median=round(med["sylsp"], 4), unpack_bytes_per_entry=24,
                   unpack_gb_per_s=round(24 * n / med["sylsp"] / 1e6, 1),
                   note="unpack: 12 B read + 12 B written per entry (8 B k-mer + 4 B count); no share of peak is stated")
        if kind == "shuffled":
            rec.update(sort_ms=[round(x, 4) for x in ms["sort"]], sort_ms_median=round(med["sort"], 4),
                       sort_bytes_per_entry_per_pass=24, dedup_ms=[round(x, 4) for x in ms["sylsp_dedup"]], dedup_ms_median=round(med["sylsp_dedup"], 4),
                       dedup_bytes_per_entry=8 + 4 + 4 + 4 + 12 + 4 + 4 + 12,
                       sort_road_note="sort: rocPRIM's stable radix sort of (8 B key, 4 B value) pairs over all 64 key bits, 12 B read + 12 B written per entry "
                                      "and pass (the number of passes is rocPRIM's choice); dedup: flags 8 B read + 4 B written, exclusive sum 4 B + 4 B, "
                                      "compaction 12 B + 4 B + 4 B read and 12 B written per entry")
        emit(rec)
        del dev
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=64)
    ap.add_argument("--entries", type=int, default=1_900_000, help="entries per sketch (the table of a 1 Gbp pair at c = 200: about 1.9 M)")
    ap.add_argument("--genomes", type=int, default=1000, help="genomes of the synthetic database")
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
