"""The read kernel carries two 32-bit stream bases per lane through its hash loop (record_geometry, csrc/reads_block.h; the arithmetic:
csrc/seed_plan.h, tests/test_pass_state_plan.py) where it carried four 64-bit offsets, reloads its k-mer count from LDS behind the loop,
indexes records in 32 bits and ranks a pair's survivors by compares.  What can go wrong there is a matter of record lengths, of which
mate a lane holds, of where the batch lies in memory and of which pass and push a record belongs to, so the samples — about 600 pairs,
a few blocks each — are:

  * lengths:  records of 0, 30, 31, 32, 33, 65, 66, 150, 151 and 400 bases in random order: every side of every marker rule (a single
              read wants 66..400 bases, a pair 33 in both mates), mates too short to hash, and records at the halo's length;
  * long401:  the same with one record of 401 bases: the read kernel declines the batch, the position kernel gives the table;
  * halo:     2 x 150 pairs with a mate 2 on a block's first coordinate, its mate 1 in the block before (the halo);
  * ragged:   reads of 35..151 bases: every pass is dealt by length, a lane hashes another lane's record.

Each at c = 1 (spill regions, the unlisted survivors' search), 2 and 200, k = 21 and 31, single and paired, both seeding rules, ASCII
and packed input, and the three hash spellings — spelling 2 also with "reads_slack" wide enough that candidates are struck and the
pass's bookkeeping runs a second time; and every sample again from a device buffer whose base pointer is 1..15 bytes off a 16-byte
boundary, in two pushes into one session (the second push's records count on from the first's).  Every table must be the CPU
oracle's."""
import numpy as np
import pytest

import sylph_amd as S
from oracle import oracle as O

from . import seed_plan_lib as SP
from .helpers import concat, random_seq

LENGTHS = (0, 30, 31, 32, 33, 65, 66, 150, 151, 400)
NAMES = ("lengths", "long401", "halo", "ragged")
CS = (1, 2, 200)
MODES = [(S.SEED_SCALAR, O.MODE_SCALAR), (S.SEED_AVX2_COMPAT, O.MODE_AVX2_COMPAT)]
N_REC = 1200


def make_lengths(name, rng):
    if name in ("lengths", "long401"):
        lens = rng.choice(np.array(LENGTHS), size=N_REC).tolist()
        lens[:len(LENGTHS)] = LENGTHS                                   # every length at least once, whatever the draw
        lens[10:16] = (150, 32, 32, 150, 33, 33)                         # pairs with a short mate 1, a short mate 2, two mates of exactly 33
        if name == "long401":
            lens[N_REC // 2 + 1] = 401
        return lens
    if name == "halo":
        lens = [150] * N_REC
        lens[0] = lens[1] = 75                                           # every later mate 2 starts on a multiple of 300: some block's first coordinate
        lens[-2] = lens[-1] = 225
        return lens
    return rng.integers(35, 152, size=N_REC).tolist()


@pytest.fixture(scope="module", params=[(k, name) for k in (21, 31) for name in NAMES], ids=lambda p: f"k{p[0]}-{p[1]}")
def case(request):
    k, name = request.param
    rng = np.random.default_rng(1500 + 100 * k + NAMES.index(name))
    genome = random_seq(rng, 30000)
    lens = make_lengths(name, rng)
    recs = [genome[s:s + n].copy() for s, n in zip(rng.integers(0, len(genome) - 401, size=len(lens)).tolist(), lens)]
    for r in recs[::23]:
        if len(r):
            r[int(rng.integers(0, len(r)))] = ord("N")
    b, off = concat(recs)
    want = {(c, paired, om): O.sketch_reads(b, off, c=c, k=k, mode=om, paired=paired) for c in CS for paired in (False, True) for _, om in MODES}
    return dict(k=k, name=name, b=b, off=off, want=want)


def test_the_samples_are_what_they_claim(case):
    """CPU only: the lengths, the blocks, the mate 2 that opens a block, the dealt passes"""
    K = SP.constants()
    k, name, off = case["k"], case["name"], case["off"]
    lens = np.diff(off.astype(np.int64))
    n_rec = len(lens)
    assert n_rec == N_REC and int(off[-1]) <= 300 * n_rec                         # the session's gate for the read kernel
    p = SP.plan(int(off[-1]), n_rec, 0, 200, k)
    assert p["tpb"] == K["RTPB"] and 2 <= p["n_blk"] <= 8
    blk_rec, rel = SP.blocks(off, 0, p["rt"], p["n_blk"])
    if name in ("lengths", "long401"):
        assert set(LENGTHS) <= set(lens.tolist()) and (lens.max() == 401) == (name == "long401")
        pairs = lens.reshape(-1, 2)
        assert ((pairs[:, 0] < 33) & (pairs[:, 1] >= 33)).any() and ((pairs[:, 0] >= 33) & (pairs[:, 1] < 33)).any()
        assert ((pairs[:, 0] == 33) & (pairs[:, 1] == 33)).any() and ((pairs[:, 0] == 400) | (pairs[:, 1] == 400)).any()
    elif name == "halo":
        opens = [i for i in range(1, p["n_blk"]) if blk_rec[i] < n_rec and blk_rec[i] & 1 and rel[blk_rec[i]] == K["RH"]]
        assert opens, "no block starts with a mate 2 on its first coordinate"
        m2 = blk_rec[opens[0]]
        assert blk_rec[opens[0] - 1] <= m2 - 1 < blk_rec[opens[0]]                  # its mate 1 starts in the block before
    else:
        nh = np.maximum(lens - (k - 1), 0)
        first = blk_rec[:-1][np.diff(blk_rec) > 1]
        assert all(len(set(nh[a:a + 256].tolist())) > 8 for a in first.tolist())    # every pass is dealt
        assert lens.min() >= 35 and lens.max() <= 151
    for c in CS:
        assert len(case["want"][(c, True, O.MODE_AVX2_COMPAT)]["kmers"]) > (200 if c == 1 else 3 if c == 200 else 100), (name, c)


def hash_spellings(c):
    th = (0xFFFFFFFFFFFFFFFF // c) >> 32
    if c == 1:                                                                    # (spelling 2 is not for c = 1: the session takes 1)
        return [(0, 0), (1, 0), (2, 0)]
    return [(0, 0), (1, 0), (2, 0), (2, th // 3), (2, min(4 * th, 0xFFFFFFFE - th - 1))]


def sketch(ctx, pushes, **kw):
    """one session, the pushes in order -> (table, batches the read kernel took, batches the position kernel took)"""
    ctx.profile(True)
    try:
        sk = S.ReadSketcher(ctx, **kw)
        for push in pushes:
            push(sk)
        g = sk.finish()
        sk.close()
        return g, ctx.kernel_stats("short_reads")[1], ctx.kernel_stats("position_road")[1]
    finally:
        ctx.profile(False)


def same(g, e, tag):
    assert np.array_equal(g["kmers"], e["kmers"]), tag
    assert np.array_equal(g["counts"], e["counts"]), tag
    assert g["dup_removed"] == e["dup_removed"], tag


@pytest.mark.gpu
def test_tables_equal_the_oracle_over_the_grid(ctx, case):
    from sylph_amd.binding import ENC_2BIT, MEM_HOST
    k, b, off, declines = case["k"], case["b"], case["off"], case["name"] == "long401"
    packed = S.pack_2bit(b)
    try:
        for c in CS:
            for hv, slack in hash_spellings(c):
                ctx.set_option("reads_hash", str(hv))
                ctx.set_option("reads_slack", str(slack))
                for paired, (gm, om) in [(p, m) for p in (False, True) for m in MODES]:
                    e = case["want"][(c, paired, om)]
                    for enc in ("ascii", "2bit"):
                        tag = (case["name"], k, c, hv, slack, paired, gm, enc)
                        push = (lambda sk: sk.push(b, off)) if enc == "ascii" else (lambda sk: sk.push_enc(packed, off, int(off[-1]), MEM_HOST, ENC_2BIT))
                        g, took, fell_back = sketch(ctx, [push], c=c, k=k, paired=paired, seed_mode=gm)
                        assert (took, fell_back) == ((0, 1) if declines else (1, 0)), tag     # no quiet fallback; the 401-base record does fall back
                        same(g, e, tag)
    finally:
        ctx.set_option("reads_hash", "-1")
        ctx.set_option("reads_slack", "0")


@pytest.mark.gpu
def test_an_unaligned_base_pointer_and_a_second_push(ctx, case):
    """bias 1..15: the batch starts that many bytes behind a 16-byte boundary, so every stream base shifts against the block grid; the
    second push starts in the middle of the sample (on a pair's first mate) and its records count on from the first's"""
    import torch
    k, b, off, declines = case["k"], case["b"], case["off"], case["name"] == "long401"
    n = len(off) - 1
    cut = (n // 2 + 37) & ~1
    offs = [torch.from_numpy((off[a:z + 1] - off[a]).astype(np.int64)).cuda() for a, z in ((0, cut), (cut, n))]
    # the sample at every start 1..15 bytes behind a 16-byte boundary (padding behind it: the loads take whole 16-byte words)
    shifted = {bias: torch.from_numpy(np.concatenate([np.zeros(bias, np.uint8), b, np.zeros(600, np.uint8)])).cuda() for bias in range(1, 16)}
    torch.cuda.synchronize()
    biases = iter(list(range(1, 16)) * 4)
    for c in CS:
        for paired, (gm, om) in [(p, m) for p in (False, True) for m in MODES]:
            bias = next(biases)
            first = shifted[bias].data_ptr() + bias
            assert first % 16 == bias
            pushes = [lambda sk: sk.push_device(first, offs[0].data_ptr(), cut, int(off[cut])),
                      lambda sk: sk.push_device(first + int(off[cut]), offs[1].data_ptr(), n - cut, int(off[n] - off[cut]))]
            tag = (case["name"], k, c, paired, gm, bias)
            g, took, fell_back = sketch(ctx, pushes, c=c, k=k, paired=paired, seed_mode=gm)
            assert took + fell_back == 2 and (fell_back == 1) == declines, tag
            same(g, case["want"][(c, paired, om)], tag)
