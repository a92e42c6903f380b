"""Interleaved paired reads through `sylph-hip sketch --interleaved`, against the two-file command (profiles/interleaved.txt).

Whole commands (the default): bench.py's 1 Gbp pair of the README's files leg (3,333,334 pairs of 150 bp, random bases, tools/feed_bench.py
write_fastq) as two files AND as one interleaved file, plain and `gzip -1`.  Per kind: `sylph-hip sketch --interleaved F` on this
tree's binary and `sylph-hip sketch -1 A -2 B` on the binary of --parent (a directory that holds the parent commit's sylph-hip and its
two libraries; without it: this tree's binary), default flags, alternating — which goes first alternates too —, every command started
--settle seconds after the previous one exited; median of --reps runs with the spread (max - min), every `[sylph_hip feed]` lap of
every run kept (whole commands carry the GPU runtime's start-up, which varies by 0.1 s; the laps do not).  The two k-mer tables
must be equal.  One sample per command: the plain sample is a process's first and takes the indexed host feed; --warm puts a small
plain sample in front, so that the measured one takes the device route (both binaries alike).

--kernel (a run apart): the mate-check kernel alone by the library's timer (family "mate_check": HIP events around the launch), through
the binding, on the interleaved text already in device memory, with the files' 10-byte ids and with --id-bytes N (+ an Illumina-style
comment) ids.  Bytes: what the kernel reads — per pair two header walks of 32 bytes per step up to the step in which the ids end, and
32 bytes of the index (where the two headers start and end).

GPU box: python tools/interleaved_bench.py [--parent DIR] [--warm] [--out FILE];  python tools/interleaved_bench.py --kernel [--out FILE]"""
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
L = 150


def records(seqs, mate_tag=None, id_bytes=10):
    """(n, record bytes) array of four-line records '@r000000000' (padded with 'x' to id_bytes; mate_tag: ' 1:N:0:ACGT' behind it)"""
    n = len(seqs) // L
    head = 1 + id_bytes + (len(mate_tag) if mate_tag else 0) + 1
    rec = np.empty((n, head + L + 3 + L + 1), dtype=np.uint8)
    ids = np.arange(n)
    rec[:, 0] = ord("@")
    rec[:, 1:1 + id_bytes] = ord("x")
    rec[:, 1] = ord("r")
    for d in range(9):
        rec[:, 10 - d] = 48 + (ids // 10 ** d) % 10
    if mate_tag:
        rec[:, 1 + id_bytes:head - 1] = np.frombuffer(mate_tag, dtype=np.uint8)
    rec[:, head - 1] = 10
    rec[:, head:head + L] = seqs.reshape(n, L)
    rec[:, head + L:head + L + 3] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, head + L + 3:head + 2 * L + 3] = ord("I")
    rec[:, -1] = 10
    return rec


def mates_of(mbp, seed=1):
    rng = np.random.default_rng(seed)
    n = int(mbp * 1e6) // L
    return [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n * L)] for _ in (1, 2)], n


def interleave(r1, r2):
    return np.stack([r1, r2], axis=1).reshape(-1)


def table_of(path):
    with open(path, "rb") as f:
        raw = f.read()
    n = int.from_bytes(raw[:8], "little")
    return raw[:8 + 12 * n], raw[8 + 12 * n:]


def commands(a, emit):
    d = tempfile.mkdtemp(prefix="sylph_interleaved_")
    try:
        seqs, n = mates_of(a.mbp)
        r = [records(s) for s in seqs]
        for m in (0, 1):
            r[m].tofile(f"{d}/s_{m + 1}.fq")
        interleave(r[0], r[1]).tofile(f"{d}/s_il.fq")
        small = [records(s[:20000 * L]) for s in seqs]
        for m in (0, 1):
            small[m].tofile(f"{d}/w_{m + 1}.fq")
        interleave(small[0], small[1]).tofile(f"{d}/w_il.fq")
        del r, seqs
        jobs = [subprocess.Popen(["gzip", "-1", "-k", "-f", f"{d}/{f}.fq"]) for f in ("s_1", "s_2", "s_il")]
        assert all(j.wait() == 0 for j in jobs)
        gbp = 2 * n * L / 1e9
        new_exe = os.path.join(ROOT, "sylph_amd", "sylph-hip")
        base_exe = os.path.join(a.parent, "sylph-hip") if a.parent else new_exe
        emit(dict(what="one interleaved file (this tree) against two files (baseline)", pairs=n, gbp=round(gbp, 4), reps=a.reps, settle_seconds=a.settle,
                  warm_sample_in_front=bool(a.warm), baseline="the parent commit's binary" if a.parent else "this tree's binary",
                  bytes={f: os.path.getsize(f"{d}/{f}") for f in ("s_1.fq", "s_il.fq", "s_1.fq.gz", "s_il.fq.gz")},
                  header_bytes_in_the_interleaved_file=2 * n * 12))
        laps = {}

        def run(exe, kind, il):
            env = dict(os.environ, SYLPH_HIP_FEED_TRACE="1")
            for k in ("SYLPH_HIP_EXACT_DEDUP", "SYLPH_HIP_INFLATE_STREAM", "SYLPH_HIP_FEED_DEVICE"):
                env.pop(k, None)
            sfx = "fq.gz" if kind == "gzip" else "fq"
            out = f"{d}/out_{'il' if il else 'two'}"
            shutil.rmtree(out, ignore_errors=True)
            if il:
                args = ["--interleaved"] + ([f"{d}/w_il.fq"] if a.warm else []) + [f"{d}/s_il.{sfx}"]
            else:
                args = ["-1"] + ([f"{d}/w_1.fq"] if a.warm else []) + [f"{d}/s_1.{sfx}", "-2"] + ([f"{d}/w_2.fq"] if a.warm else []) + [f"{d}/s_2.{sfx}"]
            time.sleep(a.settle)
            t = time.perf_counter()
            p = subprocess.run([exe, "sketch", "-t", "1"] + args + ["-d", out], capture_output=True, text=True, env=env, timeout=1200)
            dt = time.perf_counter() - t
            if p.returncode != 0:
                raise RuntimeError(p.stderr[-800:])
            laps.setdefault((kind, il), []).append([(m.group(1).strip(), float(m.group(2))) for m in re.finditer(r"\[sylph_hip feed\] (.*?)\s+([0-9.]+) ms", p.stderr)])
            return dt, table_of(f"{out}/{'s_il' if il else 's_1'}.{sfx}.paired.sylsp")

        run(new_exe, "plain", True)                                          # untimed: the binaries, the libraries and the files come off the disk
        run(base_exe, "plain", False)
        laps.clear()
        for kind in a.kinds.split(","):
            new, base, same = [], [], True
            for rep in range(a.reps):
                order = (True, False) if rep % 2 == 0 else (False, True)
                got = {}
                for il in order:
                    got[il] = run(new_exe if il else base_exe, kind, il)
                new.append(got[True][0])
                base.append(got[False][0])
                same = same and got[True][1][0] == got[False][1][0]
                print(f"# {kind} rep {rep}: interleaved {new[-1]:.3f} s, two files {base[-1]:.3f} s", flush=True)
            med_n, med_b = float(np.median(new)), float(np.median(base))
            emit(dict(kind=kind, interleaved_seconds=[round(x, 3) for x in new], two_file_seconds=[round(x, 3) for x in base],
                      interleaved_median=round(med_n, 3), interleaved_spread=round(max(new) - min(new), 3), two_file_median=round(med_b, 3),
                      two_file_spread=round(max(base) - min(base), 3), interleaved_gbp_per_s=round(gbp / med_n, 3), two_file_gbp_per_s=round(gbp / med_b, 3),
                      interleaved_median_within_two_file_min_max=bool(min(base) <= med_n <= max(base)), tables_equal=same,
                      interleaved_laps_ms=laps[(kind, True)], two_file_laps_ms=laps[(kind, False)]))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def kernel(a, emit):
    import torch

    import sylph_amd as S
    from sylph_amd.binding import MEM_DEVICE
    seqs, n = mates_of(a.mbp)
    ctx = S.Context(0)
    ctx.profile(True)
    for id_bytes, tags in ((10, (None, None)), (a.id_bytes, (b" 1:N:0:ACGTACGT", b" 2:N:0:ACGTACGT"))):
        text = interleave(records(seqs[0], tags[0], id_bytes), records(seqs[1], tags[1], id_bytes))
        dev = torch.from_numpy(text).cuda()
        torch.cuda.synchronize()
        f = S.FastqText(ctx, dev.data_ptr(), MEM_DEVICE, len(text))
        pairs = f.n_records // 2
        ms = []
        for rep in range(a.reps + 1):                                        # (the first repetition is not counted)
            t0 = ctx.kernel_stats("mate_check")[0]
            assert f.mates() == pairs
            ctx.synchronize()
            if rep:
                ms.append(ctx.kernel_stats("mate_check")[0] - t0)
        f.close()
        steps = id_bytes // 32 + 1                                           # the step in which the id ends (its end byte is at id_bytes)
        header_bytes, index_bytes = pairs * 2 * 32 * steps, pairs * 32
        med = float(np.median(ms))
        emit(dict(what="mates_kernel alone, by the library's timer", pairs=pairs, id_bytes=id_bytes, header_line_bytes=len(tags[0] or b"") + id_bytes + 2,
                  steps_per_pair=steps, ms=[round(x, 4) for x in ms], ms_median=round(med, 4), header_bytes_read=header_bytes, index_bytes_read=index_bytes,
                  gb_per_s=round((header_bytes + index_bytes) / med / 1e6, 1),
                  note="bytes the lanes ask for: 32 per header and step + 32 of index per pair; the cache lines behind them are more (a header "
                       "lies every ~320 bytes of text).  No share of peak is stated."))
        del dev
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=500, help="bases per mate (bench.py's pair: 500)")
    ap.add_argument("--kinds", default="plain,gzip")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--settle", type=float, default=2.0)
    ap.add_argument("--parent", default="", help="directory with the parent commit's sylph-hip, libsylph_host.so and libsylph_hip.so")
    ap.add_argument("--warm", action="store_true", help="a small plain sample in front of the measured one (it then takes the device route)")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--id-bytes", type=int, default=36)
    ap.add_argument("--out", default="", help="append the JSON lines to this file too")
    a = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    (kernel if a.kernel else commands)(a, emit)


if __name__ == "__main__":
    main()
