"""The FASTA index and join (csrc/fasta.hip) alone: a synthetic FASTA text of --mb megabytes that already lies in device memory — at
line width 60, and as one line per record — indexed (sylph_fasta_index with SYLPH_MEM_DEVICE: wall clock of the call, its read-backs
included) and joined (the join kernel's time between two events, family "fasta_join"; the join is run through sylph_fasta_bases of the
text's first, one-base record, which joins the whole text on the device and copies one byte back).  GB/s are bytes of TEXT per second.
One JSON line per shape.  GPU box: python tools/fasta_bench.py [--mb 1000] [--reps 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sylph_amd as S  # noqa: E402
from sylph_amd.binding import MEM_DEVICE  # noqa: E402


def make_text(mb, width, record_bases=4_000_000, seed=1):
    """records of record_bases bases (a 64 Mbp random block repeated) behind one record of one base; width 0 = one line per record"""
    rng = np.random.default_rng(seed)
    block = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=64_000_000)]
    per_record = record_bases + (record_bases // width if width else 1) + 32
    n_rec = max(1, int(mb * 1e6) // per_record)
    parts = [b">first\nA\n"]
    for r in range(n_rec):
        seq = block[(r * record_bases) % (len(block) - record_bases):][:record_bases]
        parts.append(b">record_%d synthetic\n" % r)
        if width:
            lines = np.full((record_bases // width, width + 1), 10, dtype=np.uint8)
            lines[:, :width] = seq[:record_bases // width * width].reshape(-1, width)
            parts.append(lines.tobytes())
        else:
            parts.append(seq.tobytes() + b"\n")
    return b"".join(parts), n_rec + 1


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = S.Context(0)
    ctx.profile(True)
    for what, width in (("line width 60", 60), ("one line per record", 0)):
        text, n_rec = make_text(a.mb, width)
        dev = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        pad = torch.zeros(64, dtype=torch.uint8, device="cuda")     # (readable bytes behind the text, whatever the allocator does)
        torch.cuda.synchronize()
        index_ms, join_ms = [], []
        n_bases = 0
        for rep in range(a.reps + 1):                                # (the first repetition pays for the allocations: not counted)
            t = time.perf_counter()
            f = S.FastaText(ctx, dev.data_ptr(), MEM_DEVICE, len(text))
            dt = time.perf_counter() - t
            before = ctx.kernel_stats("fasta_join")[0]
            assert f.n_records == n_rec and f.bases(0, 1).tobytes() == b"A"
            jt = ctx.kernel_stats("fasta_join")[0] - before
            n_bases = f.n_bases
            f.close()
            if rep:
                index_ms.append(dt * 1e3)
                join_ms.append(jt)
        gb = len(text) / 1e9
        print(json.dumps(dict(what=what, text_bytes=len(text), records=n_rec, bases=n_bases, reps=a.reps,
                              index_ms_median=round(float(np.median(index_ms)), 3), index_ms_min=round(min(index_ms), 3), index_ms_max=round(max(index_ms), 3),
                              join_ms_median=round(float(np.median(join_ms)), 3), join_ms_min=round(min(join_ms), 3), join_ms_max=round(max(join_ms), 3),
                              index_text_gb_per_s=round(gb / (np.median(index_ms) / 1e3), 1), join_text_gb_per_s=round(gb / (np.median(join_ms) / 1e3), 1),
                              index_and_join_text_gb_per_s=round(gb / ((np.median(index_ms) + np.median(join_ms)) / 1e3), 1))), flush=True)
        del dev, pad
    ctx.close()


if __name__ == "__main__":
    main()
