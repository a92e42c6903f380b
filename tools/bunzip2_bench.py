"""Device bzip2 decoder (csrc/bunzip2.hip) alone: bench.py's mate file shape (150 bp reads; constant or --qual binned qualities, text from
inflate_bench.make_text) compressed with bzip2 at each --levels level, decoded through sylph_bunzip2: wall clock of the call (H2D of the
compressed bytes included), the kernel families' times (sylph_ctx_kernel_stats), GB/s of text, bytes checked against Python's bz2 —
which is also the reference's decoder on the reference's one thread, timed on the same file in the same run.  One JSON line per
(file, level).  The file is compressed by --jobs processes as one bzip2 stream per 64 MiB piece (pbzip2's layout; `bzip2` itself
would take ~4 min per level for 1 Gbp): the device decodes the streams' blocks side by side either way."""
import argparse
import bz2
import json
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sylph_amd as S  # noqa: E402
from inflate_bench import make_text  # noqa: E402

FAMILIES = ["bunzip2_scan", "bunzip2_decode", "bunzip2_bwt", "bunzip2_walk", "bunzip2_rle", "bunzip2_crc"]
PIECE = 64 << 20


def _compress(job):
    path, off, n, level = job
    with open(path, "rb") as f:
        f.seek(off)
        return bz2.compress(f.read(n), level)


def compress_file(path, level, jobs):
    size = os.path.getsize(path)
    with Pool(jobs) as pool:
        parts = pool.map(_compress, [(path, o, min(PIECE, size - o), level) for o in range(0, size, PIECE)])
    out = f"{path}.{level}.bz2"
    with open(out, "wb") as f:
        for p in parts:
            f.write(p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=1000)
    ap.add_argument("--levels", default="9,1")
    ap.add_argument("--qual", default="const", choices=["const", "binned"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--no-host", action="store_true", help="skip the one-thread libbz2 decode (and the byte check)")
    a = ap.parse_args()
    path = make_text(a.mbp, a.qual, 1)
    text_bytes = os.path.getsize(path)
    ctx = S.Context(0)
    ctx.profile(True)
    for lv in a.levels.split(","):
        t = time.perf_counter()
        p = compress_file(path, int(lv), a.jobs)
        t_compress = time.perf_counter() - t
        data = np.fromfile(p, dtype=np.uint8)
        best = None
        for rep in range(a.reps):
            before = {f: ctx.kernel_stats(f)[0] for f in FAMILIES}
            t = time.perf_counter()
            b = S.Bunzipped(ctx, data)
            dt = time.perf_counter() - t
            fam = {f: round(ctx.kernel_stats(f)[0] - before[f], 3) for f in FAMILIES}
            rec = dict(what=f"bzip2 -{lv} (one stream per {PIECE >> 20} MiB piece)", qual=a.qual, mbp=a.mbp, text_bytes=text_bytes,
                       bz_bytes=int(len(data)), ratio=round(text_bytes / len(data), 2), call_ms=round(dt * 1e3, 2),
                       text_gb_per_s=round(text_bytes / dt / 1e9, 2), kernel_ms=fam, kernel_ms_sum=round(sum(fam.values()), 3),
                       streams=b.n_members, blocks=b.n_blocks, candidates=b.n_candidates, compress_s=round(t_compress, 1), rep=rep)
            if rep == 0:
                got = b.read().tobytes()
            b.close()
            if best is None or rec["call_ms"] < best["call_ms"]:
                best = rec
        if not a.no_host:
            t = time.perf_counter()
            expect = bz2.decompress(data.tobytes())           # libbz2 on this one thread: the reference's decoder and thread count
            best["libbz2_one_thread_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            best["bytes_equal_bz2"] = bool(got == expect)
            best["speedup_vs_libbz2"] = round(best["libbz2_one_thread_ms"] / best["call_ms"], 1)
            del expect
        del got
        print(json.dumps(best), flush=True)
        os.remove(p)


if __name__ == "__main__":
    main()
