"""FASTA-format read files through `sylph-hip sketch`, device routes against the host reader (profiles/fasta_reads_device.txt).

Whole commands (the default): bench.py's 1 Gbp pair (3,333,334 pairs of 150 bp, random bases) written as FASTA, one line per record
unless --width says otherwise, as a plain pair, a `gzip -1` pair, a `bzip2 -9` pair, and the gzip pair streamed
(SYLPH_HIP_INFLATE_STREAM=1).  Per kind: `sylph-hip sketch -1 .. -2 ..` with default flags on this tree's binary with
SYLPH_HIP_FASTA_READS_DEVICE=1, and on the binary of --parent (a directory that holds the parent commit's sylph-hip and its two
libraries), which knows no device route for FASTA reads and takes the host reader: the same files, alternating, every command started
--settle seconds after the previous one exited; median of --reps runs with the spread (max - min).  Without --parent the baseline is
this tree's binary with SYLPH_HIP_FASTA_READS_DEVICE=0, and the file says so.  A kind ships on by default only if its median beats the
baseline's by more than the two spreads together.

--kernels (a run apart): the join (family "fasta_join") and the gather (family "fasta_batch") by the library's timers, through the
binding, on the same pair's text already in device memory; GB/s against their algorithmic bytes: join 1 B read + 1 B written per base,
gather 1 B read + 1 B written per base + 4 B of offsets per record.

--same-route (with --parent; profiles/read_text_refactor.txt): for a change that must leave speed alone.  The baseline binary runs
with the device routes ON too, the kinds fastq_plain, fastq_gzip and fastq_gzip_streamed (the same pair as FASTQ, bench.py's files leg
and the stream's) join the list, and every `[sylph_hip feed]` lap of every run is kept: whole commands carry the GPU runtime's
start-up, which varies by 0.1 s; the laps do not.

GPU box: python tools/fasta_reads_bench.py [--parent DIR [--same-route]] [--out FILE];  python tools/fasta_reads_bench.py --kernels [--out FILE]"""
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


def write_fasta(path, seqs, L, width):
    """n = len(seqs) / L records '>r000000000' of L bases, `width` bases per line (0: one line)"""
    n = len(seqs) // L
    w = width if width else L
    lines = (L + w - 1) // w
    rec = np.full((n, 12 + L + lines), 10, dtype=np.uint8)
    ids = np.arange(n)
    rec[:, 0] = ord(">")
    rec[:, 1] = ord("r")
    for d in range(9):
        rec[:, 10 - d] = 48 + (ids // 10 ** d) % 10
    s = seqs.reshape(n, L)
    for j in range(lines):
        a, b = j * w, min(L, (j + 1) * w)
        rec[:, 12 + a + j:12 + b + j] = s[:, a:b]
    rec.tofile(path)
    return rec.nbytes


def make_pair(d, mbp, width, seed, kinds):
    rng = np.random.default_rng(seed)
    L = 150
    n = int(mbp * 1e6) // L
    for m in (1, 2):
        seqs = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n * L)]
        write_fasta(f"{d}/s_{m}.fa", seqs, L, width)
        if any(k.startswith("fastq") for k in kinds):
            from feed_bench import write_fastq
            write_fastq(f"{d}/s_{m}.fq", seqs, L)
    jobs = []
    if "gzip" in kinds or "gzip_streamed" in kinds:
        jobs += [subprocess.Popen(["gzip", "-1", "-k", "-f", f"{d}/s_{m}.fa"]) for m in (1, 2)]
    if "fastq_gzip" in kinds or "fastq_gzip_streamed" in kinds:
        jobs += [subprocess.Popen(["gzip", "-1", "-k", "-f", f"{d}/s_{m}.fq"]) for m in (1, 2)]
    if "bzip2" in kinds:
        jobs += [subprocess.Popen(["bzip2", "-9", "-k", "-f", f"{d}/s_{m}.fa"]) for m in (1, 2)]
    while any(j.poll() is None for j in jobs):
        time.sleep(20)
        print("# compressing ...", flush=True)
    assert all(j.returncode == 0 for j in jobs)
    return n


def commands(a, emit):
    kinds = a.kinds.split(",") + (["fastq_plain", "fastq_gzip", "fastq_gzip_streamed"] if a.same_route and a.kinds == ap_default_kinds else [])
    d = tempfile.mkdtemp(prefix="sylph_fasta_reads_")
    try:
        n = make_pair(d, a.mbp, a.width, 1, kinds)
        gbp = 2 * n * 150 / 1e9
        new_exe = os.path.join(ROOT, "sylph_amd", "sylph-hip")
        base_exe = os.path.join(a.parent, "sylph-hip") if a.parent else new_exe
        emit(dict(what="FASTA read pair", pairs=n, gbp=round(gbp, 4), line_width=a.width or "one line per record", reps=a.reps, settle_seconds=a.settle,
                  bytes={k: os.path.getsize(f"{d}/s_1.fa{s}") for k, s in (("plain", ""), ("gzip", ".gz"), ("bzip2", ".bz2")) if os.path.exists(f"{d}/s_1.fa{s}")},
                  baseline=("the parent commit's binary, device routes on" if a.same_route else "the parent commit's binary (host reader)") if a.parent
                  else "this tree's binary with SYLPH_HIP_FASTA_READS_DEVICE=0 (host reader)"))
        suffix = {"plain": "fa", "gzip": "fa.gz", "bzip2": "fa.bz2", "gzip_streamed": "fa.gz", "fastq_plain": "fq", "fastq_gzip": "fq.gz", "fastq_gzip_streamed": "fq.gz"}
        laps = {}

        def run(exe, kind, device):
            env = dict(os.environ, SYLPH_HIP_FEED_TRACE="1", SYLPH_HIP_FASTA_READS_DEVICE=device)
            env.pop("SYLPH_HIP_EXACT_DEDUP", None)
            env.pop("SYLPH_HIP_INFLATE_STREAM", None)
            if kind.endswith("gzip_streamed"):
                env["SYLPH_HIP_INFLATE_STREAM"] = "1"
            out = f"{d}/out_{'new' if exe == new_exe else 'base'}_{device}"
            time.sleep(a.settle)
            t = time.perf_counter()
            p = subprocess.run([exe, "sketch", "-1", f"{d}/s_1.{suffix[kind]}", "-2", f"{d}/s_2.{suffix[kind]}", "-d", out],
                               capture_output=True, text=True, env=env, timeout=1200)
            dt = time.perf_counter() - t
            if p.returncode != 0:
                raise RuntimeError(p.stderr[-800:])
            route = "FASTA device route" if ("FASTA records" in p.stderr) else "device route" if "device route:" in p.stderr else "host reader"
            laps.setdefault((kind, exe), []).append({m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"\[sylph_hip feed\] (.*?)\s+([0-9.]+) ms", p.stderr)})
            with open(f"{out}/s_1.{suffix[kind]}.paired.sylsp", "rb") as f:
                return dt, route, f.read()

        run(new_exe, "plain", "1")                                           # untimed: the binary, the libraries and the runtime's files come off the disk
        laps.clear()
        for kind in kinds:
            new, base, routes, same = [], [], set(), True
            for rep in range(a.reps):
                first_new = not (a.same_route and rep % 2)                   # --same-route: which binary goes first alternates too
                if first_new:
                    dt, route, sk_new = run(new_exe, kind, "1")
                dt_b, route_b, sk_base = run(base_exe, kind, "1" if a.same_route else "0")
                if not first_new:
                    dt, route, sk_new = run(new_exe, kind, "1")
                new.append(dt)
                routes.add(route)
                base.append(dt_b)
                assert route_b == (route if a.same_route else "host reader")
                same = same and sk_new == sk_base
                print(f"# {kind} rep {rep}: {new[-1]:.3f} s against {base[-1]:.3f} s", flush=True)
            med_n, med_b = float(np.median(new)), float(np.median(base))
            spread_n, spread_b = max(new) - min(new), max(base) - min(base)
            emit(dict(kind=kind, route=sorted(routes), device_seconds=[round(x, 3) for x in new], baseline_seconds=[round(x, 3) for x in base],
                      device_median=round(med_n, 3), device_spread=round(spread_n, 3), baseline_median=round(med_b, 3), baseline_spread=round(spread_b, 3),
                      device_gbp_per_s=round(gbp / med_n, 3), baseline_gbp_per_s=round(gbp / med_b, 3), speedup=round(med_b / med_n, 2),
                      sketches_byte_identical=same, on_by_default=bool(routes == {"FASTA device route"} and same and med_n + spread_n + spread_b < med_b),
                      **(dict(device_median_within_baseline_min_max=bool(min(base) <= med_n <= max(base)), device_laps_ms=laps[(kind, new_exe)],
                              baseline_laps_ms=laps[(kind, base_exe)]) if a.same_route else {})))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def kernels(a, emit):
    import torch

    import sylph_amd as S
    from sylph_amd.binding import MEM_DEVICE
    d = tempfile.mkdtemp(prefix="sylph_fasta_reads_")
    try:
        n = make_pair(d, a.mbp, a.width, 1, [])
        texts = [np.fromfile(f"{d}/s_{m}.fa", dtype=np.uint8) for m in (1, 2)]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    ctx = S.Context(0)
    ctx.profile(True)
    dev = [torch.from_numpy(t).cuda() for t in texts]
    pad = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    join_ms, batch_ms = [], []
    bases = 0
    for rep in range(a.reps + 1):                                            # (the first repetition pays for the allocations: not counted)
        f = [S.FastaText(ctx, t.data_ptr(), MEM_DEVICE, len(t)) for t in dev]
        bases = f[0].n_bases + f[1].n_bases
        sk = S.ReadSketcher(ctx, c=200, paired=True, dedup_fpr=1e-4)
        j0, b0 = ctx.kernel_stats("fasta_join")[0], ctx.kernel_stats("fasta_batch")[0]
        sk.push_fasta(f[0], f[1])
        ctx.synchronize()
        jt, bt = ctx.kernel_stats("fasta_join")[0] - j0, ctx.kernel_stats("fasta_batch")[0] - b0
        sk.finish()
        sk.close()
        for x in f:
            x.close()
        if rep:
            join_ms.append(jt)
            batch_ms.append(bt)
    del dev, pad
    jm, bm = float(np.median(join_ms)), float(np.median(batch_ms))
    emit(dict(what="kernel times by the library's timers (HIP events around the launches), one paired push of the whole pair", pairs=n, bases=bases,
              line_width=a.width or "one line per record", reps=a.reps,
              join_ms=[round(x, 3) for x in join_ms], join_ms_median=round(jm, 3), join_bytes=2 * bases, join_gb_per_s=round(2 * bases / jm / 1e6, 1),
              gather_ms=[round(x, 3) for x in batch_ms], gather_ms_median=round(bm, 3), gather_bytes=2 * bases + 8 * n,
              gather_gb_per_s=round((2 * bases + 8 * n) / bm / 1e6, 1),
              note="join: both files' launches summed, 1 B read + 1 B written per base (the text's headers and line ends it also reads are not counted); "
                   "gather: 1 B read + 1 B written per base + 4 B of offsets per record.  No share of peak is stated."))
    ctx.close()


ap_default_kinds = "plain,gzip,bzip2,gzip_streamed"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=500, help="bases per mate (bench.py's pair: 500)")
    ap.add_argument("--width", type=int, default=0, help="bases per FASTA line (0: one line per record)")
    ap.add_argument("--kinds", default=ap_default_kinds)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--settle", type=float, default=2.0)
    ap.add_argument("--parent", default="", help="directory with the parent commit's sylph-hip, libsylph_host.so and libsylph_hip.so")
    ap.add_argument("--same-route", action="store_true", help="the baseline binary takes the device routes too, FASTQ kinds are added, laps are kept")
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
