"""reads_kernel builds a k-mer and its reverse complement right-aligned with clean tops and takes the smaller with ONE v_min_f64
(kmer_step, csrc/reads.hip; min_u62, csrc/device_common.h): below 2^62 the order of doubles is the order of their bits.  The reads here
put in front of that instruction what random reads hardly ever do — denormal and zero operands (k-mers that begin with five or more A;
every 21-mer), the largest exponents (TTTTT.. on both strands), pairs of windows whose high words are equal — at every stream alignment
and every place of a group of 16, through single and paired sessions, ASCII and packed input and the three hash spellings; the sample
table must be the CPU oracle's, entry for entry, at c = 1 (every k-mer is in the table) and c = 7.

A k-mer and its reverse complement cannot differ in the LAST base only: position i differs exactly when position k - 1 - i does, and for
odd k the middle base always does.  The latest place where the two can part is therefore the middle base (`late_split`, both orders);
k-mers that differ from one another in nothing but their last base (so their reverse complements in nothing but the first) are here too.

The same sequences as one record above the read kernel's 400 bases and through sketch_genomes take the position kernel."""
import numpy as np
import pytest

import sylph_amd as S
from oracle import oracle as O

from .helpers import concat, random_seq, revcomp

MODES = [(S.SEED_SCALAR, O.MODE_SCALAR), (S.SEED_AVX2_COMPAT, O.MODE_AVX2_COMPAT)]


def seq(s):
    return np.frombuffer(s.encode(), dtype=np.uint8).copy()


def engineered_kmers(k, rng):
    """k-mers as base arrays, each followed in the list by its reverse complement (so either strand is the smaller one somewhere)."""
    out = []

    def rnd(n):
        return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))

    out += [seq("A" * k), seq("T" * k)]                                   # zero on one strand, 2^2k - 1 on the other
    for n_a in (1, 4, 5, 6, 16, 26, 31):                                  # canonical form starts with n_a A: denormal from 5 A on
        n_a = min(n_a, k)
        for _ in range(3):
            body = "A" * n_a + ("C" + rnd(k) if n_a < k else "")
            km = seq(body[:k - 1] + "A") if n_a < k else seq(body)        # last base A: the other strand starts with T
            out += [km, revcomp(km)]
    for _ in range(4):                                                    # TTTTT.. on both strands: the largest exponents
        km = seq("TTTTT" + rnd(k - 10) + "AAAAA")
        out += [km, revcomp(km)]
    half = (k - 1) // 2
    for _ in range(6):                                                    # late_split: equal up to the middle base; for k = 31 the right-aligned
        x = rnd(half)                                                     # windows have equal high words (15 bases) and the low word decides
        for mid in "ACGT":
            out.append(np.concatenate([seq(x + mid), revcomp(seq(x))]))
    hi_bases = k - 16                                                     # bases in the high word of a right-aligned window
    for _ in range(6):                                                    # equal high words, the low words apart anywhere
        x = rnd(min(hi_bases, half))
        mid = rnd(k - 2 * len(x))
        km = np.concatenate([seq(x + mid), revcomp(seq(x))])
        out += [km, revcomp(km)]
    for _ in range(4):                                                    # k-mers that differ in their last base only
        stem = rnd(k - 1)
        for last in "ACGT":
            km = seq(stem + last)
            out += [km, revcomp(km)]
    return out


def engineered_records(k, seed):
    """-> (records, number of the sweep's records).  The sweep: every length from k to k + 47 eight times, in an order under which the
    records' starts fall on all 16 alignments of a stream word; then every engineered k-mer at two places of a read."""
    rng = np.random.default_rng(seed)
    recs = []
    for rep in range(8):
        for j in range(48):
            recs.append(random_seq(rng, k + (j * 7 + rep) % 48))
    n_sweep = len(recs)
    for i, km in enumerate(engineered_kmers(k, rng)):
        for lead in (i % 17, 47 - i % 31):
            tail = int(rng.integers(0, 48 - lead))
            recs.append(np.concatenate([random_seq(rng, lead), km, random_seq(rng, tail)]).astype(np.uint8))
    if len(recs) % 2:
        recs.append(random_seq(rng, k + 11))
    return recs, n_sweep


@pytest.fixture(scope="module", params=[21, 31])
def case(request):
    k = request.param
    recs, n_sweep = engineered_records(k, 6200 + k)
    b, off = concat(recs)
    want = {(c, paired, om): O.sketch_reads(b, off, c=c, k=k, mode=om, paired=paired)
            for c in (1, 7) for paired in (False, True) for _, om in MODES}
    return dict(k=k, recs=recs, n_sweep=n_sweep, b=b, off=off, want=want)


def test_the_reads_cover_what_they_claim(case):
    """CPU only: alignments, lengths, and the operands of the minimum."""
    k, recs, off = case["k"], case["recs"], case["off"]
    assert 300 <= len(recs) <= 900 and len(recs) % 2 == 0
    assert {int(o) % 16 for o in off[:case["n_sweep"]]} == set(range(16))
    assert {len(r) for r in recs[:case["n_sweep"]]} == set(range(k, k + 48))
    assert all(k <= len(r) <= k + 47 for r in recs)
    code = np.zeros(256, dtype=np.int64)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
    lead_a, both_t, hi_equal, late = set(), 0, 0, 0
    hb = 2 * k - 32
    for r in recs[case["n_sweep"]:]:
        c = code[r].tolist()
        for s in range(len(c) - k + 1):
            f = rc = 0
            for j in range(k):
                f = (f << 2) | c[s + j]
                rc = (rc << 2) | (3 - c[s + k - 1 - j])
            m = min(f, rc)
            lead_a.add(k - (m.bit_length() + 1) // 2)
            both_t += (f >> (2 * k - 10)) == 0x3FF and (rc >> (2 * k - 10)) == 0x3FF
            hi_equal += (f >> 32) == (rc >> 32) and f != rc and (f >> 32) != 0
            late += (f ^ rc).bit_length() <= k + 1                     # equal down to the middle base
            assert f < (1 << 62) and rc < (1 << 62) and (f >> 32) < (1 << hb)
    assert {5, 16, min(26, k), min(31, k), k} <= lead_a                # k leading A: the operand 0
    assert both_t >= 4 and hi_equal >= 12 and late >= 12


def sketch(ctx, case, c, paired, gm, packed=None):
    from sylph_amd.binding import ENC_2BIT, MEM_HOST
    sk = S.ReadSketcher(ctx, c=c, k=case["k"], paired=paired, seed_mode=gm)
    if packed is None:
        sk.push(case["b"], case["off"])
    else:
        sk.push_enc(packed, case["off"], int(case["off"][-1]), MEM_HOST, ENC_2BIT)
    r = sk.finish()
    sk.close()
    return r


@pytest.mark.gpu
def test_read_kernel_tables_equal_the_oracle(ctx, case):
    packed = S.pack_2bit(case["b"])
    try:
        for hv in (0, 1, 2):
            ctx.set_option("reads_hash", str(hv))
            for c in (1, 7):
                for paired in (False, True):
                    for gm, om in MODES:
                        e = case["want"][(c, paired, om)]
                        assert len(e["kmers"]) > (2000 if c == 1 else 200)
                        for enc, p in (("ascii", None), ("2bit", packed)):
                            g = sketch(ctx, case, c, paired, gm, p)
                            tag = (case["k"], hv, c, paired, gm, enc)
                            assert np.array_equal(g["kmers"], e["kmers"]), tag
                            assert np.array_equal(g["counts"], e["counts"]), tag
                            assert g["dup_removed"] == e["dup_removed"], tag
    finally:
        ctx.set_option("reads_hash", "-1")


@pytest.mark.gpu
def test_position_kernel_roads_equal_the_oracle(ctx, case):
    """One record of all the sequences (longer than the read kernel takes) and the records as the contigs of a genome."""
    k = case["k"]
    joined = np.concatenate(case["recs"]).astype(np.uint8)
    assert len(joined) > 400
    joff = np.array([0, len(joined)], dtype=np.uint64)
    for gm, om in MODES:
        for c in (1, 7):
            e = O.sketch_reads(joined, joff, c=c, k=k, mode=om, paired=False)
            sk = S.ReadSketcher(ctx, c=c, k=k, paired=False, seed_mode=gm)
            sk.push(joined, joff)
            g = sk.finish()
            sk.close()
            assert np.array_equal(g["kmers"], e["kmers"]) and np.array_equal(g["counts"], e["counts"]), (k, c, gm)
            # two genomes: the one long contig, and every record as a contig of its own
            b2, off2 = concat([joined] + case["recs"])
            goff = np.array([0, 1, 1 + len(case["recs"])], dtype=np.uint64)
            km, koff, tr, toff = ctx.sketch_genomes(b2, off2, goff, c=c, k=k, seed_mode=gm)
            for gi in range(2):
                lo, hi = int(goff[gi]), int(goff[gi + 1])
                gb = b2[int(off2[lo]):int(off2[hi])]
                go = (off2[lo:hi + 1] - off2[lo]).astype(np.uint64)
                eg = O.sketch_genome(gb, go, c=c, k=k, mode=om)
                assert np.array_equal(km[int(koff[gi]):int(koff[gi + 1])], eg["genome_kmers"]), (k, c, gm, gi)
                assert np.array_equal(tr[int(toff[gi]):int(toff[gi + 1])], eg["tracked"]), (k, c, gm, gi)
