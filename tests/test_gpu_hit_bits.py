"""The read kernel sets a k-mer's hit bit with an LDS xor under the threshold compare's own lane mask (kmer_step, csrc/reads_block.h;
the encoding and its decode: csrc/seed_plan.h, tests/test_hit_bits_plan.py).  What can go wrong there is a matter of WHERE a record ends
inside the words of its mask column and of who writes the column, so the batches are:

  * equally long reads whose last unit is a single k-mer, a lone half-group (in the upper and in the lower half of a word), an even
    group, an odd group: k-mer counts 1, 8, 16, 24, 32, 40 (k = 31: lengths 31, 38, 46, 54, 62, 70), and 150 / 151 bp;
  * ragged reads: the pass is dealt by length, a lane xors into ANOTHER lane's column (slot != tid), lanes idle behind their wave's
    longest read write beyond their record's own words;
  * tiny reads, more than 256 to a block: two passes, the columns zeroed again in between.

Each at c = 1 (every bit set, both halves of every word full: the decode's worst case), 2 and 200, single and paired, ASCII and packed
input, k = 21 and 31, and the three hash spellings — spelling 2 with "reads_slack" wide enough that candidates are struck and the
bookkeeping redone (on words that must then be decoded already) in every pass that has k-mers to spare.  Every table must be the CPU
oracle's, and the context's counters must say that the read kernel took the batch."""
import numpy as np
import pytest

import sylph_amd as S
from oracle import oracle as O

from .helpers import concat, random_seq

N_KMERS = (1, 8, 16, 24, 32, 40)
NAMES = [f"nh{n}" for n in N_KMERS] + ["len150", "len151", "ragged", "tiny"]
CS = (1, 2, 200)
# the scalar rule hashes every k-mer of a read (the counts above are exact); the default rule whole fours of them (a 151 bp read ends
# in a lone half-group either way, a read of one k-mer hashes nothing: a wavefront without a loop)
MODES = [(S.SEED_SCALAR, O.MODE_SCALAR), (S.SEED_AVX2_COMPAT, O.MODE_AVX2_COMPAT)]


def draw(rng, genome, lengths):
    return [genome[s:s + n].copy() for s, n in zip(rng.integers(0, len(genome) - 400, size=len(lengths)).tolist(), lengths)]


def make_batch(name, k, rng):
    genome = random_seq(rng, 40000)
    if name.startswith("nh"):
        lengths = [k - 1 + int(name[2:])] * 2600
    elif name.startswith("len"):
        lengths = [int(name[3:])] * 2600
    elif name == "ragged":
        lengths = rng.integers(k - 4, 152, size=3000).tolist()            # some too short to hash at all
    else:
        # tiny: four in five without a single k-mer, so that a block of the smallest size holds more than 256 records
        lengths = np.where(rng.random(6000) < 0.8, rng.integers(0, 11, size=6000), rng.integers(k, k + 40, size=6000)).tolist()
    recs = draw(rng, genome, lengths)
    if name == "ragged":
        for r in recs[::17]:
            r[int(rng.integers(0, len(r)))] = ord("N")
    return recs


@pytest.fixture(scope="module", params=[(k, name) for k in (21, 31) for name in NAMES], ids=lambda p: f"k{p[0]}-{p[1]}")
def case(request):
    k, name = request.param
    recs = make_batch(name, k, np.random.default_rng(1400 + 100 * k + NAMES.index(name)))
    b, off = concat(recs)
    want = {(c, paired, om): O.sketch_reads(b, off, c=c, k=k, mode=om, paired=paired) for c in CS for paired in (False, True) for _, om in MODES}
    return dict(k=k, name=name, recs=recs, b=b, off=off, want=want)


def test_the_batches_are_what_they_claim(case):
    """CPU only: where the records end, that ragged passes are ragged and that tiny reads fill a block more than once."""
    from . import seed_plan_lib as SP
    k, name, off = case["k"], case["name"], case["off"]
    n_rec = len(off) - 1
    assert 2000 <= n_rec <= 6000 and n_rec % 2 == 0
    nh = np.maximum(np.diff(off.astype(np.int64)) - (k - 1), 0)
    assert int(off[-1]) <= 300 * n_rec and nh.max() <= 152 - k
    if name.startswith("nh"):
        assert set(nh.tolist()) == {int(name[2:])}
    elif name.startswith("len"):
        assert set(nh.tolist()) == {int(name[3:]) - k + 1}
    else:
        p = SP.plan(int(off[-1]), n_rec, 0, 200, k)
        blk_rec, _ = SP.blocks(off, 0, p["rt"], p["n_blk"])
        per_block = np.diff(blk_rec)
        assert p["tpb"] == 256
        if name == "tiny":
            assert per_block.max() > 256 and (per_block > 256).sum() >= 3          # a second pass, its columns zeroed again
            assert set(range(1, 41)) <= set(nh.tolist())                          # every place a record's last unit can end
        else:
            first = blk_rec[:-1][per_block > 1]
            assert all(len(set(nh[a:a + 256].tolist())) > 8 for a in first.tolist())   # every pass is dealt
            assert len(set(((nh + 7) // 8).tolist())) >= 15                        # every number of half-groups up to 150 bp
    for c in CS:
        assert len(case["want"][(c, False, O.MODE_SCALAR)]["kmers"]) > (200 if c == 1 else 3 if c == 200 else 100), (name, c)


def hash_spellings(c):
    th = (0xFFFFFFFFFFFFFFFF // c) >> 32
    if c == 1:                                                                    # (spelling 2 is not for c = 1: the session takes 1)
        return [(0, 0), (1, 0), (2, 0)]
    return [(0, 0), (1, 0), (2, 0), (2, th // 3), (2, min(4 * th, 0xFFFFFFFE - th - 1))]


@pytest.mark.gpu
def test_tables_equal_the_oracle_and_the_read_kernel_ran(ctx, case):
    from sylph_amd.binding import ENC_2BIT, MEM_HOST
    k, b, off = case["k"], case["b"], case["off"]
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
                        ctx.profile(True)
                        try:
                            sk = S.ReadSketcher(ctx, c=c, k=k, paired=paired, seed_mode=gm)
                            if enc == "ascii":
                                sk.push(b, off)
                            else:
                                sk.push_enc(packed, off, int(off[-1]), MEM_HOST, ENC_2BIT)
                            g = sk.finish()
                            sk.close()
                            took, fell_back = ctx.kernel_stats("short_reads")[1], ctx.kernel_stats("position_road")[1]
                        finally:
                            ctx.profile(False)
                        assert (took, fell_back) == (1, 0), tag                    # no quiet fallback to the position kernel
                        assert np.array_equal(g["kmers"], e["kmers"]), tag
                        assert np.array_equal(g["counts"], e["counts"]), tag
                        assert g["dup_removed"] == e["dup_removed"], tag
    finally:
        ctx.set_option("reads_hash", "-1")
        ctx.set_option("reads_slack", "0")
