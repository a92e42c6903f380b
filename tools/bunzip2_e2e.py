"""Whole-command record for bzip2 input: `sylph-hip sketch -1 -2` on bench.py's 1 Gbp pair shape (inflate_bench.make_text, two seeds) as
bzip2 -9 (one stream per 64 MiB piece, compressed by --jobs processes: pbzip2's layout), gzip -6 (one member per 64 MiB piece, the same
way) and plain files: the median of --runs runs, --gap seconds apart, per input kind, and whether the three .sylsp tables are equal."""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bunzip2_bench import PIECE, compress_file  # noqa: E402
from inflate_bench import make_text  # noqa: E402

BIN = os.path.join(ROOT, "sylph_amd", "sylph-hip")


def _gz(job):
    path, off, n = job
    with open(path, "rb") as f:
        f.seek(off)
        return gzip.compress(f.read(n), 6)


def gzip_file(path, jobs):
    from multiprocessing import Pool
    size = os.path.getsize(path)
    with Pool(jobs) as pool:
        parts = pool.map(_gz, [(path, o, min(PIECE, size - o)) for o in range(0, size, PIECE)])
    out = path + ".gz"
    with open(out, "wb") as f:
        for p in parts:
            f.write(p)
    return out


def table(d):
    (f,) = [os.path.join(d, x) for x in os.listdir(d)]
    raw = open(f, "rb").read()
    n = int.from_bytes(raw[:8], "little")
    return raw[: 8 + 12 * n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--gap", type=float, default=2.0)
    ap.add_argument("--jobs", type=int, default=16)
    a = ap.parse_args()
    m1, m2 = make_text(a.mbp, "const", 1), make_text(a.mbp, "const", 2)
    kinds = {"plain": (m1, m2), "gzip -6": (gzip_file(m1, a.jobs), gzip_file(m2, a.jobs)),
             "bzip2 -9": (compress_file(m1, 9, a.jobs), compress_file(m2, 9, a.jobs))}
    tables = {}
    for kind, (f1, f2) in kinds.items():
        times = []
        for r in range(a.runs):
            time.sleep(a.gap)
            out = tempfile.mkdtemp(prefix="sylph_bz_e2e_")
            t = time.perf_counter()
            p = subprocess.run([BIN, "sketch", "-1", f1, "-2", f2, "-d", out], capture_output=True, text=True, timeout=900)
            times.append(time.perf_counter() - t)
            if p.returncode:
                print(p.stderr[-3000:], file=sys.stderr)
                raise SystemExit(p.returncode)
            tables[kind] = table(out)
        times.sort()
        print(json.dumps(dict(kind=kind, mbp_per_mate=a.mbp, bytes=[os.path.getsize(f1), os.path.getsize(f2)], runs_s=[round(x, 3) for x in times],
                              median_s=round(times[len(times) // 2], 3))), flush=True)
    print(json.dumps(dict(tables_equal=len(set(tables.values())) == 1)), flush=True)


if __name__ == "__main__":
    main()
