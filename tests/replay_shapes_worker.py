"""One process per shape of the dedup tail (the switches are read once per process): samples whose buckets take every road of the
replay — 256 slots, 512 / 1024 slots, the device-wide path, the tiny-sample comparison path — exact set and filter, pairs and
single-end, one batch (the seeding kernel's slots) and three, each table against the oracle.  Started by test_gpu_replay_shapes.py."""
import sys

import numpy as np

import sylph_amd as S
from oracle import oracle as O

from .helpers import concat, random_seq, revcomp
from .test_gpu_parity import _sketch_gpu_once, assert_same_sketch, make_reads


def check(ctx, b, off, paired, c, batches, tag, **dedup):
    if dedup:       # the filter dedup (pairs): the oracle's model of the filter with the same rate and capacity
        e = O.sketch_reads_cuckoo_model(b, off, c=c, fpr=dedup["dedup_fpr"], initial_capacity=dedup["dedup_capacity"])
    else:
        e = O.sketch_reads(b, off, c=c, paired=paired)
    assert_same_sketch(_sketch_gpu_once(ctx, b, off, paired, False, S.SEED_AVX2_COMPAT, c, 31, batches, **dedup), e, tag)
    return e


def main():
    ctx = S.Context(0)
    rng = np.random.default_rng(7)
    # ordinary buckets (256 slots): duplicates, mates on one k-mer, ragged reads
    genome = random_seq(rng, 300000)
    b, off = concat(make_reads(rng, genome, 12000, 150, dup_frac=0.15, paired=True, insert=300))
    for paired in (True, False):
        for batches in (1, 3):
            check(ctx, b, off, paired, 20, batches, f"ordinary paired={paired} batches={batches}")
    check(ctx, b, off, True, 20, 1, "ordinary filter", dedup_fpr=0.05, dedup_capacity=3000)
    # k-mers 130 and 300 deep among ordinary ones: the 512- and 1024-slot configurations, with partial marker overlaps and mates without markers
    ctx.set_option("finish", "bucket")
    try:
        for depth in (130, 300):
            g = random_seq(rng, 400)
            n_pairs = depth * 400 // 160
            recs = make_reads(rng, g, n_pairs, 100, err=0.002, dup_frac=0.2, paired=True, insert=180, ragged=False)
            for _ in range(n_pairs // 10):
                j = 2 * int(rng.integers(0, len(recs) // 2))
                s0 = int(rng.integers(0, len(g) - 100))
                recs += [recs[j].copy(), revcomp(g[s0:s0 + 100])]
            for _ in range(n_pairs // 10):
                s0 = int(rng.integers(0, len(g) - 100))
                recs += [g[s0:s0 + 100].copy(), g[s0 + 5:s0 + 5 + 31].copy()]
            recs += make_reads(rng, random_seq(rng, 40000), 2000, 100, dup_frac=0.1, paired=True, insert=300, ragged=False)
            pairs = [(recs[i], recs[i + 1]) for i in range(0, len(recs), 2)]
            order = rng.permutation(len(pairs))
            db, doff = concat([m for i in order for m in pairs[i]])
            for paired in (True, False):
                for batches in (1, 3):
                    check(ctx, db, doff, paired, 7, batches, f"depth {depth} paired={paired} batches={batches}")
            check(ctx, db, doff, True, 7, 1, f"depth {depth} filter", dedup_fpr=0.05, dedup_capacity=2500)
    finally:
        ctx.set_option("finish", "auto")
    # a k-mer 2,500 deep: its bucket takes the device-wide path
    recs = make_reads(rng, genome, 8000, 150, dup_frac=0.1) + [genome[1000:1200].copy() for _ in range(2500)]
    order = rng.permutation(len(recs))
    mb, moff = concat([recs[i] for i in order])
    ctx.profile(True)
    try:
        for paired in (False, True):
            assert check(ctx, mb, moff, paired, 20, 1, f"device-wide paired={paired}")["counts"].max() > 1024
        assert ctx.kernel_stats("replay_overflow")[1] >= 1
    finally:
        ctx.profile(False)
    # a tiny sample (few buckets over the whole hash range: the comparison path of the replay)
    tb, toff = concat(make_reads(rng, random_seq(rng, 3000), 300, 120, dup_frac=0.3, paired=True, insert=250))
    for paired in (True, False):
        check(ctx, tb, toff, paired, 3, 1, f"tiny paired={paired}")
    ctx.close()
    print("replay shapes ok")


if __name__ == "__main__":
    sys.exit(main())
