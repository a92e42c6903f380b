"""Inputs shared by the streamed bzip2 decoder's tests (test_bunzip2_stream_plan.py on the CPU, test_gpu_bunzip2_stream.py and
test_gpu_cli_bzip2_stream.py on the device): texts made from seeds, once per process, and a few bit-level helpers.  Python's bz2 (libbz2)
is the expected output everywhere; no .bz2 file is committed."""
import bz2
import functools

import numpy as np

BLOCK_MAGIC = 0x314159265359
EOS_MAGIC = 0x177245385090


def fastq_text(rng, n_records, read_len=150):
    out = []
    qa = np.frombuffer(b"FFFFFFFF:,#", dtype=np.uint8)
    for i in range(n_records):
        L = read_len if isinstance(read_len, int) else int(rng.integers(read_len[0], read_len[1]))
        seq = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=L, p=[0.2495, 0.2495, 0.2495, 0.2495, 0.002])
        q = rng.choice(qa, size=L)
        out.append(b"@A00123:45:HXXXXXXXX:1:%d:%d:%d 1:N:0:ACGT\n" % (1101 + i // 9000, 1000 + (i * 37) % 30000, i))
        out.append(seq.tobytes() + b"\n+\n" + q.tobytes() + b"\n")
    return b"".join(out)


def fasta_reads_text(rng, n_records, read_len=150):
    out = []
    for i in range(n_records):
        L = read_len if isinstance(read_len, int) else int(rng.integers(read_len[0], read_len[1]))
        seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=L)
        out.append(b">read%d\n" % i + seq.tobytes() + b"\n")
    return b"".join(out)


def runs_text(rng, n_segments):
    """Random bases between runs of exactly 4, 5, 255, 259 and 260 equal bytes (and some longer): the run-length stage's edges, at
    level 1 many of them across block boundaries."""
    parts = []
    for _ in range(n_segments):
        parts.append(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.integers(1, 120))).tobytes())
        parts.append(bytes([int(rng.choice(np.frombuffer(b"ACGTF#", dtype=np.uint8)))]) * int(rng.choice([4, 5, 255, 259, 260, 1000, 3])))
    return b"".join(parts)


@functools.lru_cache(maxsize=None)
def texts():
    """fastq: ~1.2 MB of four-line FASTQ (at -1 about 13 blocks of ~25 kB compressed); fastq2: a shorter second mate; noise: 300 kB
    (at -1 three blocks of ~100 kB, each larger than a 64 KiB slice; at -9 one of ~300 kB); runs: the run-length edges"""
    rng = np.random.default_rng(2024)
    return {"fastq": fastq_text(rng, 3300), "fastq2": fastq_text(rng, 2100, read_len=(40, 250)),
            "noise": rng.integers(0, 256, size=300_000, dtype=np.uint8).tobytes(), "runs": runs_text(rng, 6000)}


@functools.lru_cache(maxsize=None)
def packed(name, level):
    return bz2.compress(texts()[name], level)


def magic_bits(data, magic=BLOCK_MAGIC):
    """every bit offset at which the 48-bit magic stands in data (true block starts; a false one has odds 2^-48 per bit)"""
    x = int.from_bytes(data, "big")
    pat = magic.to_bytes(6, "big")
    found = []
    for s in range(8):                         # the file shifted left by s bits: the magic byte-aligned
        y = (x << s).to_bytes(len(data) + 1, "big")
        i = y.find(pat)
        while i >= 0:
            found.append(8 * i - 8 + s)
            i = y.find(pat, i + 1)
    return sorted(found)


def eos_crc_bit(data):
    """bit offset of the LAST stream's combined CRC (behind its bit-aligned end-of-stream magic)"""
    x = int.from_bytes(data, "big")
    n = len(data) * 8
    for pad in range(8):
        if (x >> (pad + 32)) & ((1 << 48) - 1) == EOS_MAGIC:
            return n - pad - 32
    raise AssertionError("no end-of-stream magic")


def flip(data, bit):
    d = bytearray(data)
    d[bit // 8] ^= 0x80 >> (bit % 8)
    return bytes(d)


def block_text(data_int, n_bits, start, end):
    """the text of the block at bits [start, end) of a file (data_int: the file as one big-endian integer of n_bits), decoded by libbz2: the
    block alone in a level-9 stream of its own, whose combined CRC is the block's stored CRC"""
    body = (data_int >> (n_bits - end)) & ((1 << (end - start)) - 1)
    crc = (body >> (end - start - 80)) & 0xFFFFFFFF
    v = (((body << 48) | EOS_MAGIC) << 32) | crc
    bits = (end - start) + 80
    pad = -bits % 8
    return bz2.decompress(b"BZh9" + (v << pad).to_bytes((bits + pad) // 8, "big"))


def libbz2_prefix(data):
    """what bz2.BZ2Decompressor yields of a (damaged) file before it raises or runs out of input, stream after stream"""
    out, rest = [], data
    while rest:
        d = bz2.BZ2Decompressor()
        try:
            for i in range(0, len(rest), 4096):
                out.append(d.decompress(rest[i:i + 4096]))
                if d.eof:
                    break
        except (OSError, EOFError, ValueError):
            break
        if not d.eof:
            break
        rest = d.unused_data + rest[i + 4096:]
    return b"".join(out)
