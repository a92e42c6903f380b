"""GPU tests of the genome accumulator (csrc/genome_acc.hip; binding Context.genome_acc): one genome pushed in runs of whole contigs
must come out of the finish exactly as sylph_sketch_genome gives all contigs in one batch, and as the CPU oracle does — kept and tracked
k-mers compared as arrays — however the pushes are cut.

The input: numpy.random.default_rng(20261021); twelve contigs of 3000, 61, 2500, 0, 4000, 62, 1500, 3500, 100, 2800, 2000 and 3300
bases drawn in order from ACGT; then contig[2][700:1200] copied to contig[9][1000:1500] and its reverse complement to
contig[4][2000:2500].  The repeat's three copies lie in contigs [0,3), [3,7) and [7,12): for every c in {1, 5, 30}, k in {21, 31} and
min_spacing in {0, 30, 1000} the whole genome's sketch differs from the concatenated sketches of those three groups, so a road that
forgets duplicates across pushes fails on every combination.  (Checked on the CPU with oracle/pyref.py and the C++ oracle when this
file was written: 471-481 duplicate k-mers at c = 1, 97-107 at c = 5, 16-19 at c = 30, none inside any group.)  Every case asserts
that precondition itself from the oracle before it trusts the comparison."""
import numpy as np
import pytest

import sylph_amd as S
from oracle import oracle as O

from .helpers import concat, random_seq, revcomp

pytestmark = pytest.mark.gpu

LENS = [3000, 61, 2500, 0, 4000, 62, 1500, 3500, 100, 2800, 2000, 3300]
GROUPS = ((0, 3), (3, 7), (7, 12))
MODES = [(S.SEED_AVX2_COMPAT, O.MODE_AVX2_COMPAT), (S.SEED_SCALAR, O.MODE_SCALAR)]
CASES = [(c, k, sp) for c in (1, 5, 30) for k in (21, 31) for sp in (0, 30, 1000)]
ONE_PIECE, PER_CONTIG, AT_3_7 = [], list(range(1, 12)), [3, 7]
ERR_INVALID = -1


@pytest.fixture(scope="module")
def contigs():
    rng = np.random.default_rng(20261021)
    cs = [random_seq(rng, n) for n in LENS]
    cs[9][1000:1500] = cs[2][700:1200]
    cs[4][2000:2500] = revcomp(cs[2][700:1200])
    return cs


@pytest.fixture(scope="module")
def actx(ctx):
    """the session's context with accumulators that start at 64 seeds, so that the arrays regrow (up to nine times at c = 1)"""
    ctx.set_option("genome_acc_first_capacity", "64")
    yield ctx
    ctx.set_option("genome_acc_first_capacity", "0")


_REF = {}


def reference(ctx, contigs, c, k, gm, om, sp, pt):
    """(the library's one-batch sketch, the oracle's) of the whole genome, computed once per configuration; the oracle's must differ from
    the concatenation of the three groups' sketches, and owe that to duplicates that no group sees alone"""
    key = (c, k, gm, sp, pt)
    if key not in _REF:
        b, off = concat(contigs)
        whole = O.sketch_genome(b, off, c=c, k=k, mode=om, min_spacing=sp, pseudotax=pt)
        parts = [O.sketch_genome(*concat(contigs[a:e]), c=c, k=k, mode=om, min_spacing=sp, pseudotax=pt) for a, e in GROUPS]
        assert whole["n_dup_kmers"] > 0 and all(p["n_dup_kmers"] == 0 for p in parts)
        assert not np.array_equal(np.concatenate([p["genome_kmers"] for p in parts]), whole["genome_kmers"])
        one = ctx.sketch_genome(b, off, c=c, k=k, seed_mode=gm, min_spacing=sp, pseudotax=pt)
        assert np.array_equal(one["genome_kmers"], whole["genome_kmers"]) and np.array_equal(one["tracked"], whole["tracked"])
        if not pt:
            assert len(whole["tracked"]) == 0
        _REF[key] = (one, whole)
    return _REF[key]


def pieces(contigs, cuts):
    """the runs of whole contigs between the cut points -> [(first contig, bases, offsets)]"""
    edges = [0] + list(cuts) + [len(contigs)]
    return [(a,) + concat(contigs[a:e]) for a, e in zip(edges[:-1], edges[1:])]


def accumulate(ctx, contigs, cuts, check_counts=False, **kw):
    acc = ctx.genome_acc(**kw)
    n_contigs = n_bases = n_seeds = 0
    for first, b, off in pieces(contigs, cuts):
        acc.push(b, off)
        if check_counts:
            nc, nb, ns = acc.counts()
            n_contigs += len(off) - 1
            n_bases += int(off[-1])
            assert (nc, nb) == (n_contigs, n_bases) and ns >= n_seeds
            n_seeds = ns
    n_total = acc.counts()[2]
    out = acc.finish()
    acc.close()
    return out, n_total


def same(got, want):
    return (np.array_equal(got["genome_kmers"], want["genome_kmers"]) and np.array_equal(got["tracked"], want["tracked"])
            and got["genome_kmers"].dtype == np.uint64 and got["tracked"].dtype == np.uint64)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_any_cut_gives_the_one_batch_sketch(actx, contigs, case):
    c, k, sp = CASES[case]
    combos = [(gm, om, pt) for gm, om in MODES for pt in (True, False)]
    for gm, om, pt in combos:
        one, whole = reference(actx, contigs, c, k, gm, om, sp, pt)
        kw = dict(c=c, k=k, seed_mode=gm, min_spacing=sp, pseudotax=pt)
        for cuts in [ONE_PIECE, PER_CONTIG, AT_3_7] + [[cut] for cut in range(1, 12)]:
            got, n_seeds = accumulate(actx, contigs, cuts, check_counts=True, **kw)
            assert same(got, one) and same(got, whole), (c, k, sp, gm, pt, cuts)
            assert got["gn_size"] == sum(LENS) == whole["gn_size"] and n_seeds == whole["n_raw_seeds"]


@pytest.mark.parametrize("shift", [1, 7, 15])
def test_device_memory_at_odd_byte_offsets(actx, contigs, shift):
    """the bases as device memory that begins `shift` bytes behind an aligned allocation: every push's pointer then has its own
    alignment bias, and the bytes below it are the previous contig's bases"""
    import torch
    b, off = concat(contigs)
    dev = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), b, np.zeros(64, np.uint8)])).cuda()
    torch.cuda.synchronize()
    assert dev.data_ptr() % 256 == 0
    for (c, k, sp), (gm, om), pt in (((5, 31, 30), MODES[0], True), ((1, 21, 0), MODES[1], True), ((30, 31, 1000), MODES[0], False)):
        one, whole = reference(actx, contigs, c, k, gm, om, sp, pt)
        for cuts in (ONE_PIECE, AT_3_7, PER_CONTIG):
            acc = actx.genome_acc(c=c, k=k, seed_mode=gm, min_spacing=sp, pseudotax=pt)
            for first, pb, poff in pieces(contigs, cuts):
                acc.push(None, poff, device_ptr=dev.data_ptr() + shift + int(off[first]))
            got = acc.finish()
            acc.close()
            assert same(got, one) and same(got, whole), (shift, c, k, cuts)
    del dev


def test_edges(actx, contigs):
    c, k, sp = 5, 31, 30
    gm, om = MODES[0]
    kw = dict(c=c, k=k, seed_mode=gm, min_spacing=sp, pseudotax=True)
    # finish with no push
    acc = actx.genome_acc(**kw)
    assert acc.counts() == (0, 0, 0)
    out = acc.finish()
    acc.close()
    assert len(out["genome_kmers"]) == 0 and len(out["tracked"]) == 0 and out["gn_size"] == 0
    # pushes that hold only contigs below 2k bases (nothing is hashed in them), and a push with no contig at all
    rng = np.random.default_rng(7)
    short = [random_seq(rng, n) for n in (61, 0, 30, 2 * k - 1)]
    acc = actx.genome_acc(**kw)
    acc.push(*concat(short))
    assert acc.counts() == (4, sum(len(s) for s in short), 0)
    acc.push(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert acc.counts() == (4, sum(len(s) for s in short), 0)
    out = acc.finish()
    acc.close()
    assert len(out["genome_kmers"]) == 0 and len(out["tracked"]) == 0
    # the same pushes between real ones: the contig numbers of the later pushes continue behind them
    mixed = contigs[:3] + short + contigs[3:7] + short[:2] + contigs[7:]
    b, off = concat(mixed)
    whole = O.sketch_genome(b, off, c=c, k=k, mode=om, min_spacing=sp, pseudotax=True)
    assert whole["n_dup_kmers"] > 0
    per_contig = [O.sketch_genome(*concat([s]), c=c, k=k, mode=om, min_spacing=sp)["n_raw_seeds"] for s in mixed]
    acc = actx.genome_acc(**kw)
    done = 0
    for a, e in ((0, 3), (3, 7), (7, 7), (7, 11), (11, 13), (13, len(mixed))):
        acc.push(*concat(mixed[a:e]))
        done = e
        assert acc.counts() == (done, int(off[done]), sum(per_contig[:done]))     # counts after every push, to the seed
    out = acc.finish()
    acc.close()
    assert same(out, whole) and out["gn_size"] == whole["gn_size"]
    assert same(actx.sketch_genome(b, off, **kw), whole)


def test_errors_leave_the_accumulator_as_it_was(actx, contigs):
    c, k, sp = 5, 21, 30
    gm, om = MODES[0]
    one, whole = reference(actx, contigs, c, k, gm, om, sp, True)
    acc = actx.genome_acc(c=c, k=k, seed_mode=gm, min_spacing=sp, pseudotax=True)
    (_, b0, off0), (_, b1, off1), (_, b2, off2) = pieces(contigs, AT_3_7)

    def refused(bases, off):
        before = acc.counts()
        with pytest.raises(S.SylphHipError) as e:
            acc.push(bases, off)
        assert e.value.code == ERR_INVALID and acc.counts() == before

    refused(b0, off0 + np.uint64(1))                                       # contig_off[0] != 0
    acc.push(b0, off0)
    refused(b1, np.array([1, 5], dtype=np.uint64))
    # offsets that claim 2^32 bases over sixteen bytes of memory: refused from the offsets alone, before anything is read
    refused(np.zeros(16, np.uint8), np.array([0, 2**32], dtype=np.uint64))
    refused(np.zeros(16, np.uint8), np.array([0, 2**31, 2**32 + 5], dtype=np.uint64))
    refused(b1, np.array([0, 100, 50], dtype=np.uint64))                   # offsets that decrease
    acc.push(b1, off1)
    acc.push(b2, off2)
    got = acc.finish()
    assert same(got, one) and same(got, whole)                             # the refused pushes left nothing behind
    with pytest.raises(S.SylphHipError) as e:                              # a push after the finish
        acc.push(b0, off0)
    assert e.value.code == ERR_INVALID
    with pytest.raises(S.SylphHipError) as e:                              # ... and a second finish
        acc.finish()
    assert e.value.code == ERR_INVALID
    acc.close()
    with pytest.raises(S.SylphHipError):
        actx.genome_acc(c=5, k=25)                                         # k is 21 or 31
