"""GPU tests of FASTA text read as a sample (csrc/fasta.hip: sylph_sketch_push_fasta, sylph_fasta_index_window,
sylph_fasta_record_offset): the (k-mer, count) table and the duplicate count of a session fed from indexed FASTA text must equal, bit
for bit, those of the same records pushed as arrays (sylph_sketch_push) and those of the oracle's read sketch — for every line shape,
every alignment of the text, sub-ranges, and windows of the text fed one after the other; the window index must follow the rule the
CPU tests hold the plan header to; and what the index does not take must come back as an error that leaves the context working."""
import numpy as np
import pytest

import sylph_amd as S
from oracle import oracle as O
from sylph_amd.binding import ERR_FORMAT, MEM_DEVICE

from .fasta_texts import REFUSED, fasta_text
from .helpers import concat, random_seq, revcomp
from .test_fasta_reads_plan import TEXT, python_records, python_window
from .test_gpu_parity import MODES, assert_same_sketch

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
LENGTHS = [0, 1, 32, 33, 65, 66, 67, 399, 400, 401]


def reads_of(rng, genome, lengths, copies):
    """`copies` reads of every length (either strand, a few errors), shuffled; one in ten is an exact copy of the read in front of it"""
    recs = []
    for L in lengths * copies:
        s = int(rng.integers(0, len(genome) - L))
        m = genome[s:s + L].copy() if rng.random() < 0.5 else revcomp(genome[s:s + L])
        e = rng.random(L) < 0.005
        m[e] = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=int(e.sum()))
        recs.append(m)
    order = rng.permutation(len(recs))
    recs = [recs[i] for i in order]
    for i in range(5, len(recs), 10):
        recs[i] = recs[i - 1].copy()
    return recs


@pytest.fixture(scope="module")
def sample():
    """Two mate files over a 30 kb genome: 8 reads of every length of LENGTHS and one of 20,000 bases among them (it takes the position
    kernel and spans several output tiles), ~32 KB of bases each; mate 2 holds three records fewer.  Pairs repeat (the dedup has work)."""
    rng = np.random.default_rng(51)
    genome = random_seq(rng, 30000)
    a, b = reads_of(rng, genome, LENGTHS, 8), reads_of(rng, genome, LENGTHS[::-1], 8)
    a.insert(37, genome[5000:25000].copy())
    b.insert(37, revcomp(genome[6000:26000]))
    for i in (3, 13, 23, 43):                                  # whole pairs twice (mate 1 AND mate 2 repeat)
        a[i + 1], b[i + 1] = a[i].copy(), b[i].copy()
    b = b[:-3]
    ids_a, ids_b = [b"read%d/1 len=%d" % (i, len(r)) for i, r in enumerate(a)], [b"read%d/2 >odd @name" % i for i in range(len(b))]
    return dict(a=a, b=b, ids_a=ids_a, ids_b=ids_b, want={})


def expected(ctx, sample, paired, c, gm, om, fpr):
    """(the table of the same records pushed as arrays, the oracle's) — computed once per parameter set and shared"""
    key = (paired, c, gm, fpr)
    if key not in sample["want"]:
        n = min(len(sample["a"]), len(sample["b"]))
        recs = [x for p in zip(sample["a"][:n], sample["b"][:n]) for x in p] if paired else sample["a"]
        bases, off = concat(recs)
        sk = S.ReadSketcher(ctx, c=c, paired=paired, seed_mode=gm, **({"dedup_fpr": fpr} if fpr else {}))
        sk.push(bases, off)
        arrays = sk.finish()
        sk.close()
        oracle = O.sketch_reads_cuckoo_model(bases, off, c=c, mode=om, fpr=fpr) if fpr else O.sketch_reads(bases, off, c=c, mode=om, paired=paired)
        assert len(oracle["kmers"]) >= 200 and oracle["dup_removed"] > 0, (key, len(oracle["kmers"]), oracle["dup_removed"])
        assert_same_sketch(arrays, oracle, ("arrays against the oracle", key))
        sample["want"][key] = (arrays, oracle)
    return sample["want"][key]


PARAMS = [(paired, c, gm, om, fpr) for paired in (False, True) for c in (7, 50) for gm, om in MODES for fpr in ((0.0, 1e-4) if paired else (0.0,))]


def sketch_of(ctx, fa, fb, c, gm, fpr, pushes=None):
    sk = S.ReadSketcher(ctx, c=c, paired=fb is not None, seed_mode=gm, **({"dedup_fpr": fpr} if fpr else {}))
    if pushes is None:
        sk.push_fasta(fa, fb)
    else:
        for first, n in pushes:
            sk.push_fasta(fa, fb, first, n)
    got = sk.finish()
    sk.close()
    return got


@pytest.mark.parametrize("width,eol,last_eol,blank", [(1, b"\n", True, 0), (60, b"\n", False, 0), (60, b"\r\n", True, 7), (0, b"\n", True, 0),
                                                       (0, b"\r\n", False, 0), (1, b"\r\n", False, 50), (60, b"\n", True, 3)])
def test_sessions_fed_from_fasta_text(ctx, sample, width, eol, last_eol, blank):
    ta = fasta_text([bytes(r) for r in sample["a"]], sample["ids_a"], width=width, eol=eol, last_eol=last_eol, blank_every=blank)
    tb = fasta_text([bytes(r) for r in sample["b"]], sample["ids_b"], width=width or 60, eol=eol, last_eol=not last_eol, blank_every=blank)
    fa, fb = S.FastaText(ctx, ta), S.FastaText(ctx, tb)
    assert fa.n_records == len(sample["a"]) and fb.n_records == len(sample["b"]) and fa.n_records != fb.n_records
    for paired, c, gm, om, fpr in PARAMS:
        arrays, oracle = expected(ctx, sample, paired, c, gm, om, fpr)
        got = sketch_of(ctx, fa, fb if paired else None, c, gm, fpr)
        assert_same_sketch(got, arrays, ("arrays", width, paired, c, gm, fpr))
        assert_same_sketch(got, oracle, ("oracle", width, paired, c, gm, fpr))
    fa.close()
    fb.close()


def test_three_pushes_that_tile_the_file_give_the_table_of_one(ctx, sample):
    ta = fasta_text([bytes(r) for r in sample["a"]], sample["ids_a"], width=60)
    tb = fasta_text([bytes(r) for r in sample["b"]], sample["ids_b"], width=70)
    fa, fb = S.FastaText(ctx, ta), S.FastaText(ctx, tb)
    n = min(fa.n_records, fb.n_records)
    gm, om = MODES[1]
    for paired in (False, True):
        m = n if paired else fa.n_records
        for c, fpr in ((7, 0.0), (50, 0.0)) + (((50, 1e-4),) if paired else ()):
            arrays, _ = expected(ctx, sample, paired, c, gm, om, fpr)
            for cuts in ((0, 37, 38, m), (0, 1, m - 1, m), (0, 0, 40, m)):                # the 20,000-base record alone; single records; an empty push
                pushes = [(cuts[i], cuts[i + 1] - cuts[i]) for i in range(3)]
                got = sketch_of(ctx, fa, fb if paired else None, c, gm, fpr, pushes)
                assert_same_sketch(got, arrays, (paired, c, fpr, cuts))
    # a second session from the same indexes (their bases are joined already), and a borrowed batch whose verdict waits for finish
    arrays, _ = expected(ctx, sample, True, 50, gm, om, 0.0)
    sk = S.ReadSketcher(ctx, c=50, paired=True, seed_mode=gm)
    sk.set_option("borrow_until_finish", 1)
    sk.push_fasta(fa, fb, 0, 50)
    sk.push_fasta(fa, fb, 50, n - 50)
    assert_same_sketch(sk.finish(), arrays, "borrowed, two pushes")
    sk.close()
    fa.close()
    fb.close()


def test_device_text_at_every_misalignment(ctx, sample):
    import torch
    ta = fasta_text([bytes(r) for r in sample["a"]], sample["ids_a"], width=60, eol=b"\r\n")
    tb = fasta_text([bytes(r) for r in sample["b"]], sample["ids_b"], width=0)
    gm, om = MODES[1]
    single, _ = expected(ctx, sample, False, 7, gm, om, 0.0)
    pair, _ = expected(ctx, sample, True, 7, gm, om, 0.0)
    da = torch.zeros(len(ta) + 64, dtype=torch.uint8, device="cuda")
    db = torch.zeros(len(tb) + 64, dtype=torch.uint8, device="cuda")
    sa, sb = (torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda() for t in (ta, tb))
    assert da.data_ptr() % 16 == 0 and db.data_ptr() % 16 == 0
    for shift in range(1, 16):
        for d, s, t, other in ((da, sa, ta, shift), (db, sb, tb, 16 - shift)):
            d.fill_(ord(">") if shift & 1 else 10)                                        # junk around the text that looks like structure
            d[16 + other:16 + other + len(t)] = s
        torch.cuda.synchronize()
        fa = S.FastaText(ctx, da.data_ptr() + 16 + shift, MEM_DEVICE, len(ta))
        fb = S.FastaText(ctx, db.data_ptr() + 32 - shift, MEM_DEVICE, len(tb))
        assert_same_sketch(sketch_of(ctx, fa, None, 7, gm, 0.0), single, ("single", shift))
        assert_same_sketch(sketch_of(ctx, fa, fb, 7, gm, 0.0), pair, ("pair", shift))
        fa.close()
        fb.close()


# ------------------------------------------------------------------------------------------------------------------ the window index
def assert_holds(f, want):
    """the index holds exactly these records: [(id, sequence)]"""
    assert f.n_records == len(want) and f.n_bases == sum(len(s) for _, s in want) and f.id_bytes == sum(len(i) for i, _ in want)
    assert f.lengths().tolist() == [len(s) for _, s in want]
    assert f.ids() == [i for i, _ in want]
    assert f.bases().tobytes() == b"".join(s for _, s in want)


def ids_and_sequences(text):
    return [(text[p + 1:].split(b"\n", 1)[0].rstrip(b"\r"), s) for p, s in python_records(text)]


def test_the_window_index_at_every_cut(ctx):
    whole = S.FastaText(ctx, TEXT)
    assert_holds(whole, ids_and_sequences(TEXT))
    for cut in range(len(TEXT) + 1):
        for final in (0, 1):
            rc, n, used = python_window(TEXT[:cut], final)
            if rc:
                with pytest.raises(S.SylphHipError) as ei:
                    S.FastaText(ctx, TEXT[:cut], final=final)
                assert ei.value.code == ERR_FORMAT, (cut, final)
                continue
            f = S.FastaText(ctx, TEXT[:cut], final=final)
            assert (f.n_records, f.consumed) == (n, used), (cut, final)
            if cut % 9 == 0 or final or cut == len(TEXT):
                assert_holds(f, ids_and_sequences(TEXT[:cut] if final else TEXT[:used]))
            starts = [p for p, _ in python_records(TEXT[:cut])]
            for r in {0, n // 2, n}:
                assert f.record_offset(r) == (starts[r] if r < n else used), (cut, final, r)
            with pytest.raises(S.SylphHipError) as ei:
                f.record_offset(n + 1)
            assert ei.value.code == ERR_INVALID
            f.close()
    f = S.FastaText(ctx, TEXT, final=1)                                                  # final = 1 is sylph_fasta_index
    assert (f.n_records, f.n_bases, f.id_bytes, f.consumed) == (whole.n_records, whole.n_bases, whole.id_bytes, len(TEXT))
    assert np.array_equal(f.lengths(), whole.lengths()) and f.ids() == whole.ids() and np.array_equal(f.bases(), whole.bases())
    assert whole.record_offset(whole.n_records) == len(TEXT) and whole.record_offset(1) == python_records(TEXT)[1][0]
    f.close()
    whole.close()


def test_two_mates_walked_over_windows_of_different_sizes(ctx, sample):
    """What the stream route does: each mate's text arrives in pieces of its own size, every window is indexed (final = the text has
    ended), min(complete records) pairs are pushed, every mate keeps its text from its first record not pushed, and only the mate with
    fewer records waiting advances (both when level)."""
    texts = [fasta_text([bytes(r) for r in sample["a"]], sample["ids_a"], width=60, eol=b"\r\n", blank_every=9),
             fasta_text([bytes(r) for r in sample["b"]], sample["ids_b"], width=0, last_eol=False)]
    gm, om = MODES[1]
    for c, fpr, sizes in ((7, 0.0, (3000, 4500)), (50, 1e-4, (9000, 2500)), (50, 0.0, (100000, 1700))):
        arrays, _ = expected(ctx, sample, True, c, gm, om, fpr)
        sk = S.ReadSketcher(ctx, c=c, paired=True, seed_mode=gm, **({"dedup_fpr": fpr} if fpr else {}))
        pos, tail, advance, pushed, steps = [0, 0], [b"", b""], [True, True], 0, 0
        while True:
            steps += 1
            assert steps < 1000
            for i in range(2):
                if advance[i]:
                    tail[i] += texts[i][pos[i]:pos[i] + sizes[i]]
                    pos[i] += sizes[i]
            done = [pos[i] >= len(texts[i]) for i in range(2)]
            f = [S.FastaText(ctx, tail[i], final=int(done[i])) if (tail[i] or not done[i]) else None for i in range(2)]
            recs = [x.n_records if x else 0 for x in f]
            n = min(recs)
            if n:
                sk.push_fasta(f[0], f[1], 0, n)
                pushed += n
            for i in range(2):
                if f[i]:
                    tail[i] = tail[i][f[i].record_offset(n):]
                    f[i].close()
            if all(done) or any(done[i] and recs[i] == n for i in range(2)):
                break
            waiting = [recs[0] - n, recs[1] - n]
            advance = [not done[0] and (waiting[0] <= waiting[1] or done[1]), not done[1] and (waiting[1] <= waiting[0] or done[0])]
        assert pushed == min(len(sample["a"]), len(sample["b"])) and steps > 3
        assert_same_sketch(sk.finish(), arrays, (c, fpr, sizes))
        sk.close()


def test_what_is_refused_and_what_is_invalid(ctx, sample):
    for name, text in REFUSED.items():
        for final in (0, 1):
            if name == "empty" and final == 0:
                f = S.FastaText(ctx, text, final=0)                                       # no text yet: no records, nothing consumed
                assert (f.n_records, f.n_bases, f.consumed, f.record_offset(0)) == (0, 0, 0, 0) and f.lengths().tolist() == [] and f.ids() == []
                f.close()
                continue
            with pytest.raises(S.SylphHipError) as ei:
                S.FastaText(ctx, text, final=final)
            assert ei.value.code == ERR_FORMAT, (name, final, str(ei.value))
    one = S.FastaText(ctx, b">only a header so far", final=0)                             # one header alone: not an error
    assert (one.n_records, one.consumed) == (0, 0)
    one.close()
    end_cr = S.FastaText(ctx, b">a\nACGT\r\n>b\nAC\r", final=0)                            # a '\r' as the window's last byte lies in the kept tail
    assert (end_cr.n_records, end_cr.consumed, end_cr.bases().tobytes()) == (1, 9, b"ACGT")
    end_cr.close()
    ta = fasta_text([bytes(r) for r in sample["a"]], sample["ids_a"], width=60)
    fa = S.FastaText(ctx, ta)
    paired, single = S.ReadSketcher(ctx, c=50, paired=True), S.ReadSketcher(ctx, c=50, paired=False)
    for call in (lambda: paired.push_fasta(fa),                                          # a paired session wants both texts
                 lambda: single.push_fasta(fa, fa),                                      # ... and a single-end session one
                 lambda: single.push_fasta(fa, None, 0, fa.n_records + 1),               # more records than the file holds
                 lambda: single.push_fasta(fa, None, fa.n_records + 1, 0),
                 lambda: single.push_fasta(fa, None, 5, fa.n_records - 4)):
        with pytest.raises(S.SylphHipError) as ei:
            call()
        assert ei.value.code == ERR_INVALID, str(ei.value)
    paired.close()
    gm, om = MODES[1]
    single.push_fasta(fa)                                                                # the session and the context work afterwards
    assert_same_sketch(single.finish(), expected(ctx, sample, False, 50, gm, om, 0.0)[0], "after the refusals")
    single.close()
    fa.close()
