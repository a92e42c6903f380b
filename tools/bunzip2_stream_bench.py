"""The streamed device bzip2 decoder (csrc/bunzip2.hip sylph_bunzip2_stream_*) alone, beside tools/inflate_stream_bench.py: a synthetic
FASTQ pair of --mbp bases per mate (bench.py's shape: 150 bp reads, constant qualities) at bzip2's level 9 (one bzip2 stream per 64 MiB
piece, compressed by --jobs processes, as tools/bunzip2_bench.py makes its files), both mates in one device stream,
drained at each slice size of --slices (MiB): wall clock from open to the last window (H2D of the compressed bytes included; every window
is indexed with sylph_fastq_index_window and its complete records' text dropped, as the host's stream route does, unless --no-index), the
number of slices, the largest scratch and the largest window.  The whole-file road (sylph_bunzip2_files) on the same pair for scale.  One
JSON line per slice size; --check compares the bytes with libbz2's.  --keep DIR leaves the pair there (s_1.fq, s_1.fq.bz2, ...) for
whole-command measurements."""
import argparse
import bz2
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sylph_amd as S  # noqa: E402
from sylph_amd.binding import MEM_DEVICE  # noqa: E402


def make_pair(mbp, seed, keep, jobs):
    import feed_bench as FB
    rng = np.random.default_rng(seed)
    L = 150
    n = int(mbp * 1e6) // L
    d = keep or tempfile.mkdtemp(prefix="sylph_bunzip2_stream_")
    os.makedirs(d, exist_ok=True)
    for m in (1, 2):
        FB.write_fastq(f"{d}/s_{m}.fq", rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n * L), L)
    import bunzip2_bench as BB
    for m in (1, 2):                                       # level 9, one bzip2 stream per 64 MiB piece (pbzip2's layout), as tools/bunzip2_bench.py
        os.replace(BB.compress_file(f"{d}/s_{m}.fq", 9, jobs), f"{d}/s_{m}.fq.bz2")
    return d


def drain(ctx, bz, slice_bytes, index, check):
    """-> (seconds, info, every file's text if check)"""
    F = len(bz)
    out = [bytearray() for _ in range(F)]
    t = time.perf_counter()
    st = S.Bunzip2Stream(ctx, bz, slice_bytes)
    prev, keep = None, None
    while True:
        w = st.next(None, keep)
        if prev is not None:
            prev.close()
        prev = w
        keep = []
        for i in range(F):
            ptr, n = w.files[i]
            take = n
            if index and n:
                f = S.FastqText(ctx, ptr, MEM_DEVICE, n, final=1 if st.finished[i] else 0)
                take = n if st.finished[i] else f.consumed
                f.close()
            if check:
                out[i] += w.read_file(i)[:take]
            keep.append(take)
        if all(st.finished):
            break
    ctx.synchronize()
    dt = time.perf_counter() - t
    info = st.info()
    prev.close()
    st.close()
    return dt, info, [bytes(o) for o in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=500, help="bases per mate (bench.py's pair: 500)")
    ap.add_argument("--slices", default="16,32,64,128", help="slice sizes in MiB")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-index", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--jobs", type=int, default=16, help="processes that compress the pair")
    ap.add_argument("--keep", default=None, help="directory to make the pair in and leave it")
    a = ap.parse_args()
    d = make_pair(a.mbp, 1, a.keep, a.jobs)
    bz = [np.fromfile(f"{d}/s_{m}.fq.bz2", dtype=np.uint8) for m in (1, 2)]
    text_bytes = sum(os.path.getsize(f"{d}/s_{m}.fq") for m in (1, 2))
    expect = [bz2.decompress(b.tobytes()) for b in bz] if a.check else None
    ctx = S.Context(0)
    times = []
    for rep in range(a.reps + 1):                          # (the first call pays for the first allocations of the process)
        t = time.perf_counter()
        whole = S.Bunzipped(ctx, bz)
        times.append(time.perf_counter() - t)
        blocks = whole.n_blocks
        whole.close()
    print(json.dumps(dict(what="whole-file road (sylph_bunzip2_files)", bz_bytes=[int(len(b)) for b in bz], text_bytes=text_bytes, blocks=blocks,
                          first_ms=round(times[0] * 1e3, 2), ms=[round(x * 1e3, 2) for x in times[1:]])), flush=True)
    for mib in a.slices.split(","):
        slice_bytes = int(float(mib) * (1 << 20))
        times, info = [], None
        for rep in range(a.reps + 1):
            dt, info, got = drain(ctx, bz, slice_bytes, not a.no_index, a.check and rep == 0)
            times.append(dt)
            if a.check and rep == 0:
                assert got == expect, "the stream's bytes differ from libbz2's"
        warm = times[1:]
        rec = dict(what="stream", slice_mib=float(mib), indexed=not a.no_index, first_ms=round(times[0] * 1e3, 2), ms=[round(x * 1e3, 2) for x in warm],
                   best_ms=round(min(warm) * 1e3, 2), spread_ms=round((max(warm) - min(warm)) * 1e3, 2), text_gb_per_s=round(text_bytes / min(warm) / 1e9, 2),
                   gbp_per_s=round(2 * a.mbp / 1e3 / min(warm), 2), **info)
        if a.check:
            rec["bytes_equal_libbz2"] = True
        print(json.dumps(rec), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
