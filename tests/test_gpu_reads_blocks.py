"""The short-read kernel (csrc/reads.hip, reads_block.h) at the edges of its block geometry, every placement asserted with the plan
library (csrc/seed_plan.h through tests/seed_plan_lib.py) before the GPU is asked: (a) blocks clamped to RT_MIN with several passes each
and a 400-base record on the last and on the first coordinate of a block, (b) blocks clamped to RT_MAX with 398..400-base records among shorter ones (mean in (256, 300]: above 300 the session takes the position kernel),
(c) 2 x 150 pairs with a mate 2 on a block's first coordinate and its mate 1 in the block before.  Each batch single and paired, k = 21
and 31, c = 1 and 20, against oracle.sketch_reads: one session, one batch."""
import numpy as np
import pytest

from oracle import oracle as O

from . import seed_plan_lib as SP

pytestmark = pytest.mark.gpu

BIAS = 0          # a pushed host batch lands in a device buffer of the session's: 16-byte aligned, so the kernel's coordinates are the offsets


def offsets(lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return off


def batch_a():
    """tiny records (mean below 16: rt = RT_MIN, more than 256 records per block), a 400-base record starting on the last coordinate
    of a block and one on the first coordinate of another"""
    K = SP.constants()
    rng = np.random.default_rng(11)
    rt, lens, pos = K["RT_MIN"], [], 0

    def tiny_until(target):                 # tiny records up to exactly `target`
        nonlocal pos
        while pos < target:
            n = min(int(rng.integers(0, 25)), target - pos)
            lens.append(n)
            pos += n

    tiny_until(3 * rt - 1)
    lens.append(400); last = len(lens) - 1; pos += 400           # starts on coordinate 3 rt - 1: the last of block 2
    tiny_until(6 * rt)
    lens.append(400); first = len(lens) - 1; pos += 400          # starts on coordinate 6 rt: the first of block 6
    tiny_until(9 * rt + 77)
    if len(lens) & 1:
        lens.append(7)
    off = offsets(lens)
    p = SP.plan(int(off[-1]), len(lens), BIAS, 20, 31)
    assert p["rt"] == rt == K["RT_MIN"] and int(off[-1]) / len(lens) < 16 and 2000 <= len(lens) <= 9000
    blk_rec, rel = SP.blocks(off, BIAS, rt, p["n_blk"])
    assert np.diff(blk_rec).max() > K["RTPB"]                                        # several passes per block
    assert rel[last] == K["RH"] + rt - 1 and blk_rec[2] <= last < blk_rec[3]         # the block's last coordinate
    assert rel[first] == K["RH"] and blk_rec[6] == first                             # the block's first coordinate
    return off


def batch_b():
    """records of 398..400 bases among shorter ones, the mean in (256, 300]: rt = RT_MAX, and still a batch for the read kernel (the
    session hands batches of a mean above 300 to the position kernel)"""
    K = SP.constants()
    rng = np.random.default_rng(12)
    lens = np.where(rng.random(3200) < 0.55, rng.integers(398, 401, size=3200), rng.integers(60, 200, size=3200))
    lens[:3] = (398, 399, 400)
    off = offsets(lens)
    n_bases, n_rec = int(off[-1]), len(lens)
    p = SP.plan(n_bases, n_rec, BIAS, 20, 31)
    assert p["rt"] == K["RT_MAX"] and 256 * n_rec < n_bases <= 300 * n_rec and p["n_blk"] > 10
    assert (lens >= 398).sum() > 1000
    return off


def batch_c():
    """pairs of 2 x 150 (the first pair 2 x 75, the last 2 x 225: every later mate 2 starts on a multiple of 300): block 1 starts with a mate
    2 whose mate 1 starts in block 0"""
    K = SP.constants()
    lens = [150] * 4000
    lens[0] = lens[1] = 75
    lens[-2] = lens[-1] = 225
    off = offsets(lens)
    p = SP.plan(int(off[-1]), len(lens), BIAS, 20, 31)
    assert p["rt"] == 150 * K["RTPB"] and p["tpb"] == K["RTPB"]
    blk_rec, rel = SP.blocks(off, BIAS, p["rt"], p["n_blk"])
    b = [i for i in range(1, p["n_blk"]) if blk_rec[i] < len(lens) and blk_rec[i] & 1 and rel[blk_rec[i]] == K["RH"]]
    assert b, "no block starts with a mate 2 on its first coordinate"
    m2 = blk_rec[b[0]]
    assert blk_rec[b[0] - 1] <= m2 - 1 < blk_rec[b[0]]                               # its mate 1 starts in the block before
    return off


BATCHES = {"a_rt_min": batch_a, "b_rt_max": batch_b, "c_pairs": batch_c}


@pytest.fixture(scope="module")
def batches():
    out = {}
    for i, (name, make) in enumerate(BATCHES.items()):
        off = make()
        rng = np.random.default_rng(100 + i)
        n = int(off[-1])
        genome = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=20000).astype(np.uint8)
        # reads drawn from a small genome (so that k-mers recur and the dedup has work), with a sprinkle of N
        bases = np.empty(n, np.uint8)
        for r in range(len(off) - 1):
            a, b = int(off[r]), int(off[r + 1])
            s = int(rng.integers(0, len(genome) - 400))
            bases[a:b] = genome[s:s + b - a]
        bases[rng.integers(0, n, size=n // 500)] = ord("N")
        out[name] = (bases, off)
    return out


@pytest.mark.parametrize("c", [1, 20])
@pytest.mark.parametrize("k", [21, 31])
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_block_edges_match_the_oracle(ctx, batches, name, paired, k, c):
    import sylph_amd as S
    bases, off = batches[name]
    assert int(off[-1]) <= 300 * (len(off) - 1)                      # the session's gate for the read kernel
    ctx.profile(True)
    try:
        sk = S.ReadSketcher(ctx, c=c, k=k, paired=paired)
        sk.push(bases, off)
        r = sk.finish()
        sk.close()
        took, fell_back = ctx.kernel_stats("short_reads")[1], ctx.kernel_stats("position_road")[1]
    finally:
        ctx.profile(False)
    assert (took, fell_back) == (1, 0), (name, paired, k, c, took, fell_back)       # the read kernel did the work: no quiet fallback
    o = O.sketch_reads(bases, off, c=c, k=k, paired=paired)
    assert np.array_equal(r["kmers"], o["kmers"]) and np.array_equal(r["counts"], o["counts"]), (name, paired, k, c)
    assert r["dup_removed"] == o["dup_removed"], (name, paired, k, c)
