"""The streamed device inflate (csrc/inflate.hip sylph_inflate_stream_*) alone, modelled on tools/inflate_bench.py: a synthetic FASTQ
pair of --mbp bases per mate (bench.py's shape: 150 bp reads, constant qualities, `gzip -1`), both mates in one stream, drained at each
slice size of --slices (MiB): wall clock from open to the last window (H2D of the compressed bytes included; every window is indexed
with sylph_fastq_index_window and its complete records' text dropped, as the host's stream route does, unless --no-index), the number
of slices, the largest scratch and the largest window.  The whole-file road (sylph_inflate_files) on the same pair for scale.  One JSON
line per slice size; --check compares the bytes with zlib's."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sylph_amd as S  # noqa: E402
from sylph_amd.binding import MEM_DEVICE  # noqa: E402


def make_pair(mbp, seed):
    import feed_bench as FB
    rng = np.random.default_rng(seed)
    L = 150
    n = int(mbp * 1e6) // L
    d = tempfile.mkdtemp(prefix="sylph_inflate_stream_")
    for m in (1, 2):
        FB.write_fastq(f"{d}/s_{m}.fq", rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n * L), L)
    subprocess.run(["gzip", "-1", "-k", "-f", f"{d}/s_1.fq", f"{d}/s_2.fq"], check=True)
    return d


def drain(ctx, gz, slice_bytes, index, check):
    """-> (seconds, info, every file's text if check)"""
    F = len(gz)
    out = [bytearray() for _ in range(F)]
    t = time.perf_counter()
    st = S.InflateStream(ctx, gz, slice_bytes)
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
    ap.add_argument("--slices", default="32,64,128,256", help="slice sizes in MiB")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-index", action="store_true")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    d = make_pair(a.mbp, 1)
    gz = [np.fromfile(f"{d}/s_{m}.fq.gz", dtype=np.uint8) for m in (1, 2)]
    text_bytes = sum(os.path.getsize(f"{d}/s_{m}.fq") for m in (1, 2))
    expect = [zlib.decompress(g.tobytes(), 31) for g in gz] if a.check else None
    ctx = S.Context(0)
    times = []
    for rep in range(a.reps):
        t = time.perf_counter()
        inf = S.Inflated(ctx, gz)
        times.append(time.perf_counter() - t)
        inf.close()
    print(json.dumps(dict(what="whole-file road (sylph_inflate_files)", gz_bytes=[int(len(g)) for g in gz], text_bytes=text_bytes,
                          call_ms=[round(x * 1e3, 2) for x in times])), flush=True)
    for mib in a.slices.split(","):
        slice_bytes = int(float(mib) * (1 << 20))
        times, info = [], None
        for rep in range(a.reps):
            dt, info, got = drain(ctx, gz, slice_bytes, not a.no_index, a.check and rep == 0)
            times.append(dt)
            if a.check and rep == 0:
                assert got == expect, "the stream's bytes differ from zlib's"
        rec = dict(what="stream", slice_mib=float(mib), indexed=not a.no_index, ms=[round(x * 1e3, 2) for x in times], best_ms=round(min(times) * 1e3, 2),
                   text_gb_per_s=round(text_bytes / min(times) / 1e9, 2), gbp_per_s=round(2 * a.mbp / 1e3 / min(times), 2), **info)
        if a.check:
            rec["bytes_equal_zlib"] = True
        print(json.dumps(rec), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
