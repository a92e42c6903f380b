"""bzip2 decoded on the device (csrc/bunzip2.hip) against Python's bz2 (libbz2, the library needletail's BzDecoder wraps):
byte-identical text or a clean SYLPH_ERR_FORMAT that leaves the context usable — never different bytes.  Inputs are made here from
seeds or from the reference's three test_files/*.fasta.gz (tests/golden/ref_test_files/); no .bz2 file is committed."""
import bz2
import gzip

import numpy as np
import pytest

import sylph_amd as S
from sylph_amd.binding import ERR_FORMAT, MEM_DEVICE, SylphHipError

from .helpers import golden_bytes

pytestmark = pytest.mark.gpu


def fastq_text(rng, n_records, read_len=150, quals="binned"):
    out = []
    qa = np.frombuffer(b"FFFFFFFF:,#", dtype=np.uint8) if quals == "binned" else np.arange(33, 74, dtype=np.uint8)
    for i in range(n_records):
        L = read_len if isinstance(read_len, int) else int(rng.integers(read_len[0], read_len[1]))
        seq = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=L, p=[0.2495, 0.2495, 0.2495, 0.2495, 0.002])
        if quals == "const":
            q = np.full(L, ord("F"), dtype=np.uint8)
        elif quals == "wide":
            q = rng.choice(qa, size=L)
        else:
            q = np.repeat(rng.choice(qa, size=L // 7 + 1), 7)[:L]
        out.append(b"@A00123:45:HXXXXXXXX:1:%d:%d:%d 1:N:0:ACGT\n" % (1101 + i // 9000, 1000 + (i * 37) % 30000, i))
        out.append(seq.tobytes() + b"\n+\n" + q.tobytes() + b"\n")
    return b"".join(out)


def runs_text(rng, n_segments):
    """Random bases between runs of exactly 4, 5, 255, 259 and 260 equal bytes (and some longer): the run-length stage's edges,
    at level 1 many of them across block boundaries."""
    parts = []
    for _ in range(n_segments):
        parts.append(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.integers(1, 120))).tobytes())
        parts.append(bytes([int(rng.choice(np.frombuffer(b"ACGTF#", dtype=np.uint8)))]) * int(rng.choice([4, 5, 255, 259, 260, 1000, 3])))
    return b"".join(parts)


def decode(ctx, data):
    t = S.Bunzipped(ctx, data)
    try:
        return bytes(t.read()), t
    finally:
        t.close()


def check(ctx, data):
    expect = bz2.decompress(data)
    got, t = decode(ctx, data)
    assert len(got) == len(expect)
    assert got == expect
    return t


def test_fastq_levels(ctx):
    rng = np.random.default_rng(11)
    text = fastq_text(rng, 3000)
    for level in (1, 9):
        t = check(ctx, bz2.compress(text, level))
        assert t.n_members == 1 and t.n_blocks >= 1 and t.n_host_members == 0 and t.n_candidates >= t.n_blocks


def test_wide_qualities_ragged_reads(ctx):
    rng = np.random.default_rng(12)
    text = fastq_text(rng, 4000, read_len=(30, 400), quals="wide")
    check(ctx, bz2.compress(text, 1))
    check(ctx, bz2.compress(text, 9))


def test_runs_of_4_5_255_259_260_and_across_blocks(ctx):
    rng = np.random.default_rng(13)
    cq = fastq_text(rng, 3000, quals="const")
    check(ctx, bz2.compress(cq, 1))
    text = runs_text(rng, 12000)
    t = check(ctx, bz2.compress(text, 1))
    assert t.n_blocks >= 3
    for L in (4, 5, 255, 259, 260):
        check(ctx, bz2.compress(b"x" + b"A" * L + b"y", 9))
        check(ctx, bz2.compress(b"A" * L, 9))


def test_all_byte_values_and_one_byte_value(ctx):
    rng = np.random.default_rng(14)
    noise = rng.integers(0, 256, size=1_500_000, dtype=np.uint8).tobytes()
    assert len(set(noise)) == 256
    check(ctx, bz2.compress(noise, 9))
    check(ctx, bz2.compress(noise[:300_000], 1))
    check(ctx, bz2.compress(b"A" * 3_000_000, 9))
    check(ctx, bz2.compress(b"\x00", 9))


def test_empty_and_concatenated_streams(ctx):
    rng = np.random.default_rng(15)
    got, t = decode(ctx, bz2.compress(b"", 9))
    assert got == b"" and t.n_members == 1 and t.n_blocks == 0
    a, b = fastq_text(rng, 1500), fastq_text(rng, 800)
    data = bz2.compress(a, 1) + bz2.compress(b"", 9) + bz2.compress(b, 5) + bz2.compress(a[:5000], 2)
    t = check(ctx, data)
    assert t.n_members == 4


def test_reference_fastas_recompressed(ctx):
    for name in ("e.coli-EC590", "e.coli-K12", "e.coli-o157"):
        text = gzip.decompress(golden_bytes(f"ref_test_files/{name}.fasta.gz"))
        t = check(ctx, bz2.compress(text, 9))
        assert t.n_blocks == (len(text) + 899_999) // 900_000 or t.n_blocks >= 5


def test_more_blocks_than_compute_units_and_small_batches(ctx, monkeypatch):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(16)
    text = runs_text(rng, 100) + fastq_text(rng, 2000, quals="wide")   # (few runs: a level-1 block holds ~100 kB of this text)
    text = text * ((cus + 8) * 110_000 // len(text) + 1)
    data = bz2.compress(text, 1)
    t = check(ctx, data)
    assert t.n_blocks > cus
    monkeypatch.setenv("SYLPH_HIP_BUNZIP2_BATCH", "37")        # the chain walked across many batches of candidates
    t = check(ctx, data)
    assert t.n_blocks > cus


def test_two_files_in_one_call_and_fastq_index(ctx):
    rng = np.random.default_rng(17)
    a, b = fastq_text(rng, 5000), fastq_text(rng, 3000, read_len=(40, 250))
    t = S.Bunzipped(ctx, [bz2.compress(a, 9), bz2.compress(b, 3)])
    try:
        assert len(t.files) == 2 and t.files[0][1] == len(a) and t.files[1][1] == len(b)
        assert bytes(t.read()) == a + b
        for (ptr, n), text in zip(t.files, (a, b)):
            fq, plain = S.FastqText(ctx, ptr, MEM_DEVICE, n), S.FastqText(ctx, text)
            assert (fq.n_records, fq.n_bases) == (plain.n_records, plain.n_bases)
            assert np.array_equal(fq.lengths(), plain.lengths())
            fq.close()
            plain.close()
    finally:
        t.close()


def _eos_crc_bit(data):
    """bit offset of the stream's combined CRC (behind the bit-aligned end-of-stream magic) in a one-stream file"""
    x = int.from_bytes(data, "big")
    n = len(data) * 8
    for pad in range(8):
        if (x >> (pad + 32)) & ((1 << 48) - 1) == 0x177245385090:
            return n - pad - 32
    raise AssertionError("no end-of-stream magic")


def _flip(data, bit):
    d = bytearray(data)
    d[bit // 8] ^= 0x80 >> (bit % 8)
    return bytes(d)


def test_damaged_streams_are_declined(ctx):
    rng = np.random.default_rng(18)
    text = fastq_text(rng, 4000)
    good = bz2.compress(text, 9)
    bad = {
        "truncated": good[:-30],
        "truncated_header": good[:3],
        "symbol_bit": _flip(good, len(good) * 4 + 3),
        "block_crc": _flip(good, 4 * 8 + 48 + 5),
        "stream_crc": _flip(good, _eos_crc_bit(good) + 7),
        "trailing_garbage": good + b"not bzip2",
        "randomised": _flip(good, 4 * 8 + 48 + 32),
        "bad_header": b"BZh0" + good[4:],
        "not_bzip2": b"BZx9" + good[4:],
        "empty": b"",
    }
    for name, data in bad.items():
        with pytest.raises(SylphHipError) as e:
            S.Bunzipped(ctx, data)
        assert e.value.code == ERR_FORMAT, name
        with pytest.raises(SylphHipError) as e:
            S.Bunzipped(ctx, [good, data])
        assert e.value.code == ERR_FORMAT, name
        got, _ = decode(ctx, good)                 # the context is still usable
        assert got == text, name
