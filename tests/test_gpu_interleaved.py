"""GPU tests of interleaved paired reads at the ABI (sylph_sketch_push_fast[aq]_interleaved, sylph_fast[aq]_mates; csrc/fastq.hip,
csrc/fasta.hip, csrc/read_text.h, csrc/interleave_plan.h).  The meaning is an equivalence: a paired session fed pairs of ONE
interleaved text F must end up, bit for bit, with the table of the session fed the two mate texts A (the even records of F) and B (the
odd ones), which is the oracle's paired sketch — for FASTQ and FASTA, k 21 and 31, the exact set, the filter and no dedup, both seed
modes, any record count, any split into pushes and any cut into windows.  The mate check must name exactly the first pair of a range
whose ids are not those of mates."""
import numpy as np
import pytest

import sylph_amd as S
from oracle import oracle as O

from .fasta_texts import fasta_text
from .helpers import concat, random_seq, revcomp
from .test_gpu_parity import MODES, assert_same_sketch

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
N_PAIRS = 300                                    # more than 257: a read can go missing at pair 255, 256 and 257
C = 7


def headers_of(i):
    """the two header lines of pair i, without '@' / '>': 1 .. 90 bytes, ids unique, in the three styles that pair"""
    ident = b"%d" % i + b"x" * ((i * 7) % 58 if i >= 10 else 0)
    style = i % 3
    if i < 10 or style == 2:
        return ident, ident                                                             # the bare id, 1 byte for i < 10
    if style == 0:
        return ident + b" 1:N:0:" + b"ACGT" * (i % 6), ident + b"\t2:N:0:" + b"TG" * (i % 11)   # equal ids, cut at a space / a tab
    return ident + b"/1", ident + b"/2 left=%d" % i


def make_sample(n_pairs, seed=7):
    rng = np.random.default_rng(seed)
    genome = random_seq(rng, 30000)
    a, b = [], []
    for i in range(n_pairs):
        la, lb = int(rng.integers(31, 152)), int(rng.integers(31, 152))
        s = int(rng.integers(0, len(genome) - 600))
        ra, rb = genome[s:s + la].copy(), revcomp(genome[s + 150:s + 150 + lb])
        if i % 9 == 4:
            ra[int(rng.integers(0, la))] = ord("N")
        if i % 13 == 6:
            rb[int(rng.integers(0, lb))] = ord("N")
        a.append(ra)
        b.append(rb)
    if n_pairs > 40:
        a[11] = genome[:0].copy()                                                       # a read of 0 bp
        b[23] = genome[2000:2400].copy()                                                # ... and one of 400 bp: the read kernel's edge
        for i in (3, 30, 31, 100, 254, 255):                                            # whole pairs twice: the dedup has work
            a[i + 1], b[i + 1] = a[i].copy(), b[i].copy()
    heads = [headers_of(i) for i in range(n_pairs)]
    return dict(a=a, b=b, ha=[h[0] for h in heads], hb=[h[1] for h in heads])


def fastq_text(recs, heads, eol=b"\n", last_eol=True):
    out = []
    for i, (r, h) in enumerate(zip(recs, heads)):
        q = bytes([33 + (j * 7 + i) % 90 for j in range(len(r))])
        if i % 5 == 0 and len(r):
            q = b"@" + q[1:]                                                            # a quality line that begins like a header
        out.append(b"@" + h + eol + bytes(r) + eol + (b"+" if i % 2 else b"+" + h) + eol + q + eol)
    t = b"".join(out)
    return t if last_eol else t[:-len(eol)]


def interleaved(sample, n_records=None):
    """(records, headers) of F: A and B interleaved, cut to n_records"""
    recs = [x for p in zip(sample["a"], sample["b"]) for x in p]
    heads = [x for p in zip(sample["ha"], sample["hb"]) for x in p]
    n = len(recs) if n_records is None else n_records
    return recs[:n], heads[:n]


def text_of(kind, recs, heads, eol=b"\n"):
    return fastq_text(recs, heads, eol=eol) if kind == "fastq" else fasta_text([bytes(r) for r in recs], heads, width=70, eol=eol)


def index_of(ctx, kind, text, final=None):
    return (S.FastqText if kind == "fastq" else S.FastaText)(ctx, text, final=final)


def session(ctx, k, gm, dedup):
    kw = dict(c=C, k=k, paired=True, seed_mode=gm)
    if dedup == "filter":
        kw["dedup_fpr"] = 1e-4
    if dedup == "none":
        kw["no_dedup"] = True
    return S.ReadSketcher(ctx, **kw)


def finish(sk):
    got = sk.finish()
    sk.close()
    return got


@pytest.fixture(scope="module")
def sample():
    s = make_sample(N_PAIRS)
    s["want"] = {}
    return s


def oracle_of(sample, n_pairs, k, om, dedup):
    """the oracle's paired sketch of the first n_pairs pairs, computed once per parameter set and left unchanged"""
    key = (n_pairs, k, om, dedup)
    if key not in sample["want"]:
        recs, _ = interleaved(sample, 2 * n_pairs)
        bases, off = concat(recs) if recs else (np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
        if dedup == "filter":
            sample["want"][key] = O.sketch_reads_cuckoo_model(bases, off, c=C, k=k, mode=om, fpr=1e-4)
        else:
            sample["want"][key] = O.sketch_reads(bases, off, c=C, k=k, mode=om, paired=True, no_dedup=dedup == "none")
    return sample["want"][key]


@pytest.mark.parametrize("kind", ["fastq", "fasta"])
@pytest.mark.parametrize("k", [21, 31])
def test_interleaved_push_is_the_two_file_push_and_the_oracle(ctx, sample, kind, k):
    recs, heads = interleaved(sample)
    f = index_of(ctx, kind, text_of(kind, recs, heads))
    a = index_of(ctx, kind, text_of(kind, sample["a"], sample["ha"]))
    b = index_of(ctx, kind, text_of(kind, sample["b"], sample["hb"]))
    assert f.n_records == 2 * N_PAIRS and a.n_records == b.n_records == N_PAIRS
    assert np.array_equal(f.lengths()[0::2], a.lengths()) and np.array_equal(f.lengths()[1::2], b.lengths())   # the mean's stride
    for gm, om in MODES:
        for dedup in ("exact", "filter", "none"):
            want = oracle_of(sample, N_PAIRS, k, om, dedup)
            assert len(want["kmers"]) >= 200 and (dedup == "none" or want["dup_removed"] > 0)
            two = session(ctx, k, gm, dedup)
            (two.push_fastq if kind == "fastq" else two.push_fasta)(a, b)
            two = finish(two)
            one = session(ctx, k, gm, dedup)
            one.push_interleaved(f)
            one = finish(one)
            assert_same_sketch(one, two, ("two files", kind, k, gm, dedup))
            assert_same_sketch(one, want, ("oracle", kind, k, gm, dedup))
    for x in (f, a, b):
        x.close()


@pytest.mark.parametrize("kind", ["fastq", "fasta"])
@pytest.mark.parametrize("n_records", [0, 1, 2, 3, 2 * 255, 2 * 256 + 1])
def test_record_counts(ctx, sample, kind, n_records):
    """a last record without a mate belongs to no pair; no record at all is an index only as a window"""
    recs, heads = interleaved(sample, n_records)
    gm, om = MODES[1]
    f = index_of(ctx, kind, text_of(kind, recs, heads), final=None if n_records else 0)
    assert f.n_records == n_records
    want = oracle_of(sample, n_records // 2, 31, om, "exact")
    sk = session(ctx, 31, gm, "exact")
    sk.push_interleaved(f)
    assert_same_sketch(finish(sk), want, (kind, n_records))
    assert f.mates() == n_records // 2
    with pytest.raises(S.SylphHipError) as ei:                                           # the odd record is not half a pair
        sk = session(ctx, 31, gm, "exact")
        try:
            sk.push_interleaved(f, 0, n_records // 2 + 1)
        finally:
            sk.close()
    assert ei.value.code == ERR_INVALID
    f.close()


@pytest.mark.parametrize("kind", ["fastq", "fasta"])
def test_pushes_of_uneven_sizes(ctx, sample, kind):
    recs, heads = interleaved(sample)
    f = index_of(ctx, kind, text_of(kind, recs, heads))
    gm, om = MODES[1]
    for dedup in ("exact", "filter"):
        want = oracle_of(sample, N_PAIRS, 31, om, dedup)
        for cuts in ((0, N_PAIRS), (0, 1, N_PAIRS), (0, 0, 1, 12, 13, 256, 257, N_PAIRS)):       # 1, 2 and 7 calls (one of them empty)
            sk = session(ctx, 31, gm, dedup)
            for lo, hi in zip(cuts, cuts[1:]):
                sk.push_interleaved(f, lo, hi - lo)
            assert_same_sketch(finish(sk), want, (kind, dedup, cuts))
    sk = session(ctx, 31, gm, "exact")                                                           # one borrowed batch: the verdict waits for finish
    sk.set_option("borrow_until_finish", 1)
    sk.push_interleaved(f)
    assert_same_sketch(finish(sk), oracle_of(sample, N_PAIRS, 31, om, "exact"), (kind, "borrowed"))
    f.close()


def walk_windows(ctx, kind, text, cuts, k, gm, dedup):
    """the text arrives up to cuts[0], cuts[1], ... and then whole: every window is indexed, pairs_of(n) pairs are checked and pushed, the
    text is kept from record_offset(kept_record(n)) -> (table, pairs pushed)"""
    sk = session(ctx, k, gm, dedup)
    kept_from, pushed = 0, 0
    for end in list(cuts) + [len(text)]:
        final = int(end == len(text))
        window = text[kept_from:end]
        if not window and final:
            break
        f = index_of(ctx, kind, window, final=final)
        n = f.n_records
        pairs, kept = n // 2, 2 * (n // 2)
        assert f.mates(0, pairs) == pairs
        sk.push_interleaved(f, 0, pairs)
        at = f.record_offset(kept)
        assert at <= len(window)
        if kept < n:                                                                    # the kept tail begins at an even record of F: a mate 1
            first = window[at + 1:].split(b"\n", 1)[0].rstrip(b"\r")
            assert first == headers_of(pushed + pairs)[0], (end, first)
        pushed += pairs
        kept_from += at
        f.close()
    return finish(sk), pushed


@pytest.mark.parametrize("kind", ["fastq", "fasta"])
def test_windows_cut_at_every_byte_of_three_records(ctx, kind):
    small = make_sample(12, seed=3)
    small["want"] = {}
    recs, heads = interleaved(small)
    text = text_of(kind, recs, heads)
    gm, om = MODES[1]
    want = oracle_of(small, 12, 31, om, "exact")
    assert len(want["kmers"]) >= 50
    whole = index_of(ctx, kind, text, final=1)
    lo, hi = whole.record_offset(9), whole.record_offset(12)                            # records 9, 10, 11: a mate 2, a pair
    whole.close()
    assert 3 * 40 < hi - lo < 1500
    for cut in range(lo, hi + 1):
        got, pushed = walk_windows(ctx, kind, text, [cut], 31, gm, "exact")
        assert pushed == 12
        assert_same_sketch(got, want, (kind, cut))


@pytest.mark.parametrize("kind", ["fastq", "fasta"])
def test_windows_of_4_kib_slices(ctx, sample, kind):
    recs, heads = interleaved(sample)
    text = text_of(kind, recs, heads, eol=b"\r\n" if kind == "fasta" else b"\n")
    gm, om = MODES[1]
    for k, dedup in ((31, "exact"), (21, "filter")):
        got, pushed = walk_windows(ctx, kind, text, range(4096, len(text), 4096), k, gm, dedup)
        assert pushed == N_PAIRS
        assert_same_sketch(got, oracle_of(sample, N_PAIRS, k, om, dedup), (kind, k, dedup))


# ------------------------------------------------------------------------------------------------------------------------ the mate check
@pytest.mark.parametrize("kind", ["fastq", "fasta"])
@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
def test_mate_check(ctx, sample, kind, eol):
    recs, heads = interleaved(sample)
    f = index_of(ctx, kind, text_of(kind, recs, heads, eol=eol))
    assert f.mates() == N_PAIRS                                                         # clean: first_bad == n_pairs
    for first, n in ((0, 0), (0, 1), (1, 1), (7, 250), (255, 3), (N_PAIRS - 1, 1), (N_PAIRS, 0)):
        assert f.mates(first, n) == n, (first, n)
    for first, n in ((0, N_PAIRS + 1), (N_PAIRS + 1, 0), (N_PAIRS - 1, 2)):
        with pytest.raises(S.SylphHipError) as ei:
            f.mates(first, n)
        assert ei.value.code == ERR_INVALID
    f.close()
    # one read goes missing at pair p: pair p is mate 1 of p and mate 1 of p + 1 (or mate 2 of p and mate 1 of p + 1), and every
    # pair behind it is out of phase too.  N_PAIRS - 2 is the last pair of the shorter file.
    for p in (0, 255, 256, 257, N_PAIRS - 2):
        for mate in (0, 1):
            r, h = list(recs), list(heads)
            del r[2 * p + mate], h[2 * p + mate]
            g = index_of(ctx, kind, text_of(kind, r, h, eol=eol))
            pairs = g.n_records // 2
            assert pairs == N_PAIRS - 1
            assert g.mates() == p, (p, mate)
            assert g.mates(0, p) == p                                                   # the range in front of it is clean
            if p >= 3:
                assert g.mates(p - 3, pairs - (p - 3)) == 3                             # counted from the range's first pair
                assert g.mates(p - 3, 4) == 3 and g.mates(p - 3, 3) == 3
            if p + 1 < pairs:
                assert g.mates(p + 1, pairs - p - 1) == 0                               # a range that starts behind it: out of phase at once
            g.close()
    r, h = recs[:-1], heads[:-1]                                                        # the LAST read missing: the record in front of it has no mate
    g = index_of(ctx, kind, text_of(kind, r, h, eol=eol))
    assert g.n_records == 2 * N_PAIRS - 1 and g.mates() == N_PAIRS - 1
    g.close()


@pytest.mark.parametrize("kind", ["fastq", "fasta"])
def test_the_rule_on_headers_of_every_shape(ctx, kind):
    """ids against ids as the plan's CPU tests name them, each pair alone in a range and all in one; headers of 0 bytes and longer than a
    group's stride"""
    long_id = b"L" * 200
    cases = [(b"read7", b"read7", True), (b"read7/1", b"read7/2", True), (b"read7/2", b"read7/1", False), (b"SRR1.1", b"SRR1.2", False),
             (b"x/1", b"y/2", False), (b"/1", b"/2", True), (b"", b"", True), (b"", b"a", False), (b"a", b"", False), (b" one", b"\ttwo", True),
             (b"r 1:N:0", b"r 2:N:0", True), (b"r\t1", b"r 2", True), (b"1", b"2", False), (b"a1", b"a2", False), (b"r/1x", b"r/2x", False),
             (long_id, long_id, True), (long_id + b"/1", long_id + b"/2", True), (long_id + b"a", long_id + b"b", False),
             (long_id, long_id + b"L", False), (b"q" * 31 + b"/1", b"q" * 31 + b"/2", True), (b"q" * 30 + b"/1", b"q" * 30 + b"/2", True),
             (b"q" * 32, b"q" * 32 + b" x", True), (b"q" * 64 + b"/1 " + b"z" * 90, b"q" * 64 + b"/2", True)]
    seq = b"ACGTACGTTGCAACGTAGCTAGCTAGGATCCAGT"
    heads = [h for a, b, _ in cases for h in (a, b)]
    f = index_of(ctx, kind, text_of(kind, [np.frombuffer(seq, dtype=np.uint8)] * len(heads), heads))
    assert f.n_records == len(heads)
    verdicts = [f.mates(i, 1) == 1 for i in range(len(cases))]
    assert verdicts == [w for _, _, w in cases], [c for c, v in zip(cases, verdicts) if v != c[2]]
    assert f.mates() == [w for _, _, w in cases].index(False)
    f.close()


# ------------------------------------------------------------------------------------------------------------------------------ errors
@pytest.mark.parametrize("kind", ["fastq", "fasta"])
def test_invalid_pushes_leave_the_sessions_usable(ctx, sample, kind):
    recs, heads = interleaved(sample)
    f = index_of(ctx, kind, text_of(kind, recs, heads))
    gm, om = MODES[1]
    single = S.ReadSketcher(ctx, c=C, k=31, paired=False, seed_mode=gm)
    paired = session(ctx, 31, gm, "exact")
    paired.push_interleaved(f, 0, 100)
    for call in (lambda: single.push_interleaved(f),                                    # a single-end session
                 lambda: single.push_interleaved(f, 0, 0),
                 lambda: paired.push_interleaved(f, 100, N_PAIRS - 99),                 # 2 (first_pair + n_pairs) beyond the records
                 lambda: paired.push_interleaved(f, N_PAIRS + 1, 0),
                 lambda: paired.push_interleaved(f, 100, 2**64 - 50),
                 lambda: paired.push_interleaved(f, 0, 2**30),                          # 2 n_pairs >= 2^31
                 lambda: paired.push_interleaved(f, 100, 2**30)):
        with pytest.raises(S.SylphHipError) as ei:
            call()
        assert ei.value.code == ERR_INVALID, str(ei.value)
    paired.push_interleaved(f, 100, N_PAIRS - 100)
    assert_same_sketch(finish(paired), oracle_of(sample, N_PAIRS, 31, om, "exact"), (kind, "paired, after the refusals"))
    (single.push_fastq if kind == "fastq" else single.push_fasta)(f)                    # the single-end session takes F as what it is: reads
    bases, off = concat(recs)
    assert_same_sketch(finish(single), O.sketch_reads(bases, off, c=C, k=31, mode=om, paired=False), (kind, "single, after the refusals"))
    sk = session(ctx, 31, gm, "exact")                                                  # the same index as a and b still means: record i twice
    (sk.push_fastq if kind == "fastq" else sk.push_fasta)(f, f)
    twice = [x for r in recs for x in (r, r)]
    bases, off = concat(twice)
    assert_same_sketch(finish(sk), O.sketch_reads(bases, off, c=C, k=31, mode=om, paired=True), (kind, "a twice"))
    f.close()
