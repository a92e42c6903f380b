"""GPU tests of sylph_fasta_* (csrc/fasta.hip): the records of FASTA text found and joined on the device must be the records the host
readers find (oracle.read_fastx), byte for byte — ids, lengths and joined sequences, for every line shape and every alignment of the
text; sketches made from the indexed texts (sylph_sketch_genomes_fasta) must be the sketches of the same records concatenated on the
host; everything the index does not take must come back as SYLPH_ERR_FORMAT; and a text lent by the gzip / bzip2 decoders must index
like the plain one."""
import bz2
import zlib

import numpy as np
import pytest

import sylph_amd as S
from oracle import oracle as O
from sylph_amd.binding import ERR_FORMAT, MEM_DEVICE

from .fasta_texts import REFUSED, fasta_text, random_records, records_by_the_host_reader
from .helpers import concat, random_seq

pytestmark = pytest.mark.gpu


def the_records(rng):
    """about 40 records: a 70,000-base one (17 tiles on one line), empty ones first, in the middle and last, a 1-base one, ids with '>' and '@'"""
    recs, ids = random_records(rng, 40, max_len=10000, empty_frac=0.05)
    recs[0], recs[20], recs[-1] = b"", b"", b""
    recs[3] = bytes(random_seq(rng, 70000))
    recs[9] = b"G"
    ids[3], ids[5] = b"chr>1 @ >", b"@fastq-like >"
    return recs, ids


def text_of(recs, ids, width, eol, last_eol, trailing):
    """record 3 always on one line (it spans 17 tiles), record 6 always in 1-byte lines (tiles of nearly all newlines), blank lines inside"""
    parts = []
    for r, (seq, name) in enumerate(zip(recs, ids)):
        w = 0 if r == 3 else 1 if r == 6 else width
        parts.append(fasta_text([seq], [name], width=w, eol=eol, blank_every=5 if r % 4 == 1 else 0))
    t = b"".join(parts)
    if trailing:
        return t + eol * trailing
    return t if last_eol else t[:-len(eol)]


def assert_records(f, want):
    assert f.n_records == len(want) and f.n_bases == sum(len(s) for _, s in want) and f.id_bytes == sum(len(i) for i, _ in want)
    assert np.array_equal(f.lengths(), np.array([len(s) for _, s in want], dtype=np.uint64))
    assert f.ids() == [i for i, _ in want]
    assert f.bases().tobytes() == b"".join(s for _, s in want)
    assert f.lengths(2, 3).tolist() == [len(s) for _, s in want[2:5]] and f.ids(2, 3) == [i for i, _ in want[2:5]]
    assert f.bases(3, 4).tobytes() == b"".join(s for _, s in want[3:7]) and f.bases(0, 1).tobytes() == want[0][1]


@pytest.mark.parametrize("width", [1, 60, 80, 0])
@pytest.mark.parametrize("eol,last_eol,trailing", [(b"\n", True, 0), (b"\n", False, 0), (b"\r\n", True, 0), (b"\r\n", False, 0), (b"\n", True, 3),
                                                   (b"\r\n", True, 2)])
def test_records_of_fasta_text_found_on_the_device(ctx, tmp_path, width, eol, last_eol, trailing):
    import torch
    rng = np.random.default_rng(41)
    recs, ids = the_records(rng)
    if width == 1:
        recs = [s if r == 3 else s[:1500] for r, s in enumerate(recs)]        # (1-byte lines: keep the text near 300 KB)
    text = text_of(recs, ids, width, eol, last_eol, trailing)
    want = records_by_the_host_reader(text, tmp_path)
    assert [s for _, s in want] == recs and [i for i, _ in want] == ids
    f = S.FastaText(ctx, text)
    assert_records(f, want)
    f.close()
    # the text in device memory at byte offsets 0, 1 and 15 from a 16-byte boundary
    dev = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    assert dev.data_ptr() % 16 == 0
    for shift in (0, 1, 15):
        dev.fill_(ord(">") if shift == 1 else 10)                              # junk around the text that looks like structure
        dev[16 + shift:16 + shift + len(text)] = src
        torch.cuda.synchronize()
        f = S.FastaText(ctx, dev.data_ptr() + 16 + shift, MEM_DEVICE, len(text))
        assert_records(f, want)
        f.close()


@pytest.fixture(scope="module")
def genomes():
    """three FASTA texts: 1 contig of 200 kbp; 12 contigs of 5 to 40 kbp, one of them shorter than 2k bases and one empty; 2 contigs"""
    rng = np.random.default_rng(42)
    a = [bytes(random_seq(rng, 200000))]
    b = [bytes(random_seq(rng, int(n))) for n in rng.integers(5000, 40001, size=12)]
    b[4], b[7] = b[4][:55], b""
    c = [bytes(random_seq(rng, 30000)), a[0][1000:21000]]                        # (k-mers shared with the first genome)
    files = [(a, 60, b"\n"), (b, 80, b"\r\n"), (c, 0, b"\n")]
    texts = [fasta_text(recs, [b"contig %d" % i for i in range(len(recs))], width=w, eol=e, last_eol=(w != 80)) for recs, w, e in files]
    return [recs for recs, _, _ in files], texts


@pytest.mark.parametrize("c", [50, 200])
@pytest.mark.parametrize("pseudotax", [True, False])
def test_sketches_of_indexed_fasta_equal_the_host_batch(ctx, genomes, c, pseudotax):
    contigs, texts = genomes
    files = [S.FastaText(ctx, t) for t in texts]
    flat = [np.frombuffer(s, dtype=np.uint8) for recs in contigs for s in recs]
    bases, off = concat(flat)
    for individual in (False, True):
        goff = np.arange(len(flat) + 1, dtype=np.uint64) if individual else np.cumsum([0] + [len(r) for r in contigs]).astype(np.uint64)
        want = ctx.sketch_genomes(bases, off, goff, c=c, pseudotax=pseudotax)
        got = ctx.sketch_genomes_fasta(files, individual=individual, c=c, pseudotax=pseudotax)
        for g, w, what in zip(got, want, ("kmers", "kmer_off", "tracked", "tracked_off")):
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, individual)
        assert len(got[0]) > 0 and (len(got[2]) > 0) == pseudotax
    if c == 50 and pseudotax:                                                   # one case against the oracle: the first file alone
        k, koff, t, toff = ctx.sketch_genomes_fasta(files[:1], c=c)
        e = O.sketch_genome(flat[0], np.array([0, len(flat[0])], dtype=np.uint64), c=c)
        assert np.array_equal(k, e["genome_kmers"]) and np.array_equal(t, e["tracked"]) and koff.tolist() == [0, len(k)]
    for f in files:
        f.close()


def test_what_is_not_fasta_is_refused(ctx, tmp_path):
    import torch
    for name, text in REFUSED.items():
        with pytest.raises(S.SylphHipError) as ei:
            S.FastaText(ctx, text)
        assert ei.value.code == ERR_FORMAT, (name, str(ei.value))
        if text:                                                                # the same from device memory (nothing is decided on the host)
            dev = torch.from_numpy(np.frombuffer(text + b"\n" * 48, dtype=np.uint8).copy()).cuda()
            torch.cuda.synchronize()
            with pytest.raises(S.SylphHipError) as ei:
                S.FastaText(ctx, dev.data_ptr(), MEM_DEVICE, len(text))
            assert ei.value.code == ERR_FORMAT, (name, "device", str(ei.value))
    with pytest.raises(S.SylphHipError) as ei:                                  # 2^32 - 4096 bytes or more: refused before a byte is read
        S.FastaText(ctx, 4096, MEM_DEVICE, 2**32 - 4096)
    assert ei.value.code == ERR_FORMAT
    recs, ids = random_records(np.random.default_rng(43), 30)
    good = fasta_text(recs, ids, width=70)
    f = S.FastaText(ctx, good)                                                  # ... and the context is none the worse for it
    assert_records(f, records_by_the_host_reader(good, tmp_path))
    f.close()


def test_fasta_through_the_decoders(ctx, genomes, tmp_path):
    """gzip (level 6) and bzip2 copies of the same FASTA: decoded on the device, indexed where the decoder left them, same records, same sketch"""
    contigs, texts = genomes
    text = texts[0] + texts[1]                                                  # LF and CRLF lines, 13 records, ~460 KB, no last newline
    want = records_by_the_host_reader(text, tmp_path)
    plain = S.FastaText(ctx, text)
    want_sketch = ctx.sketch_genomes_fasta([plain], individual=True, c=50)
    plain.close()
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    gz = co.compress(text) + co.flush()
    for cls, data in ((S.Inflated, gz), (S.Bunzipped, bz2.compress(text))):
        t = cls(ctx, data)                                                      # (a decline by the decoder raises: a failure, not a skip)
        assert t.n_bytes == len(text)
        f = S.FastaText(ctx, t.dev_ptr, MEM_DEVICE, t.n_bytes)
        assert_records(f, want)
        got = ctx.sketch_genomes_fasta([f], individual=True, c=50)
        for g, w in zip(got, want_sketch):
            assert np.array_equal(g, w)
        f.close()
        t.close()
    # two files decoded in one call: each file's piece of the one text indexes on its own, at whatever address it begins
    t = S.Inflated(ctx, [gz, gz[:]])
    fs = [S.FastaText(ctx, p, MEM_DEVICE, n) for p, n in t.files]
    for f in fs:
        assert_records(f, want)
    got = ctx.sketch_genomes_fasta(fs, individual=False, c=50)
    assert got[1].tolist()[0] == 0 and len(got[1]) == 3
    for f in fs:
        f.close()
    t.close()
