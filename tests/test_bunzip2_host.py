"""bzip2 input on the CPU side: the host reader (FastxReader through libbz2, the decoder needletail 0.5.1 uses for a file that begins
with "BZ") yields exactly the records of the plain file, for FASTQ and FASTA, levels 1 and 9, files of several streams, through the
plain reader and the threaded feed; a damaged or truncated file reports an error.  And the device decoder's bookkeeping
(sylph_amd/csrc/bunzip2_plan.h, the very header csrc/bunzip2.hip includes), driven by a CPU model of the kernels' reports
(tests/bunzip2_plan_capi.cpp): the chain walk with injected false candidates, several streams and files, CRC-32/BZIP2 put together
from pieces, the run-length decode as a scan.  The checker is Python's bz2 (libbz2); the GPU side is tests/test_gpu_bunzip2.py."""
import bz2
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from .helpers import build_path, golden_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def host():
    L = C.CDLL(os.path.join(ROOT, "sylph_amd", "libsylph_host.so"))
    L.sylph_host_fastx_digest.argtypes = [C.c_char_p, C.c_int] + [C.POINTER(C.c_uint64)] * 4
    return L


@pytest.fixture(scope="module")
def plan():
    src = os.path.join(HERE, "bunzip2_plan_capi.cpp")
    out, stale = build_path("sylph_bunzip2_plan", [src] + [os.path.join(ROOT, "sylph_amd", "csrc", h) for h in ("bunzip2_plan.h", "stream_plan.h")], ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, src])
        os.replace(tmp, out)
    L = C.CDLL(out)
    L.bp_crc_raw.restype = C.c_uint32
    L.bp_crc_raw.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32]
    L.bp_crc_pieces.restype = C.c_uint32
    L.bp_crc_pieces.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64]
    L.bp_combine.restype = C.c_uint32
    L.bp_combine.argtypes = [C.POINTER(C.c_uint32), C.c_uint32]
    L.bp_rle_check.restype = C.c_longlong
    L.bp_rle_check.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64]
    L.bp_model_chain.restype = C.c_int
    L.bp_model_chain.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32,
                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32,
                                 C.c_char_p, C.c_size_t]
    return L


def fastq_text(rng, n, quals="binned"):
    out = []
    for i in range(n):
        L = int(rng.integers(0, 300)) if i % 50 else 150
        s = rng.choice(np.frombuffer(b"ACGTNacgt", dtype=np.uint8), size=L).tobytes()
        q = b"F" * L if quals == "const" else rng.choice(np.frombuffer(b"F:,#", dtype=np.uint8), size=L).tobytes()
        out.append(b"@r%d some text\n%s\n+\n%s\n" % (i, s, q))
    return b"".join(out)


def fasta_text(rng, n):
    out = []
    for i in range(n):
        s = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=int(rng.integers(1, 5000))).tobytes()
        out.append(b">c%d contig\n" % i + b"".join(s[j:j + 60] + b"\n" for j in range(0, len(s), 60)))
    return b"".join(out)


def digest(host, path, threaded):
    v = [C.c_uint64(0) for _ in range(4)]
    rc = host.sylph_host_fastx_digest(str(path).encode(), threaded, *[C.byref(x) for x in v])
    return rc, tuple(int(x.value) for x in v)


def test_bzip2_files_read_like_the_plain_file(host, tmp_path):
    rng = np.random.default_rng(7)
    texts = {"x.fq": fastq_text(rng, 4000), "c.fq": fastq_text(rng, 3000, quals="const"), "g.fa": fasta_text(rng, 300),
             "k12.fa": gzip.decompress(golden_bytes("ref_test_files/e.coli-K12.fasta.gz"))[:3_000_000]}
    for name, text in texts.items():
        plain = tmp_path / name
        plain.write_bytes(text)
        want = [digest(host, plain, t) for t in (0, 1)]
        assert want[0][0] == 0 and want[0][1][1] == 0 and want[0] == want[1]
        third = len(text) // 3
        variants = {"l1": bz2.compress(text, 1), "l9": bz2.compress(text, 9),
                    "multi": bz2.compress(text[:third], 9) + bz2.compress(b"", 1) + bz2.compress(text[third:], 2),
                    "trailing": bz2.compress(text, 5) + b"\n\x00 not another stream"}
        for v, data in variants.items():
            p = tmp_path / f"{v}.{name}.bz2"
            p.write_bytes(data)
            for threaded in (0, 1):
                assert digest(host, p, threaded) == want[0], (name, v, threaded)


def test_damaged_bzip2_reports_an_error(host, tmp_path):
    rng = np.random.default_rng(8)
    text = fastq_text(rng, 6000)
    good = bz2.compress(text, 1)
    plain = tmp_path / "p.fq"
    plain.write_bytes(text)
    _, full = digest(host, plain, 0)
    cases = {"truncated": good[: len(good) * 2 // 3], "truncated_tail": good[:-5], "flipped": bytearray(good)}
    cases["flipped"][len(good) // 2] ^= 0x10
    for name, data in cases.items():
        p = tmp_path / f"{name}.fq.bz2"
        p.write_bytes(bytes(data))
        for threaded in (0, 1):
            rc, d = digest(host, p, threaded)
            # either the file is refused up front, or its records stop with an error: never a clean digest of part of the text
            assert rc == -1 or d[1] >= 1, (name, threaded, rc, d)
            assert rc == -1 or d != full
    # a first block that cannot be decoded: the file is refused like any file that is not FASTA/FASTQ
    head = bytearray(good)
    head[12] ^= 0xFF
    p = tmp_path / "head.fq.bz2"
    p.write_bytes(bytes(head))
    assert digest(host, p, 0)[0] == -1


def _bitwise_crc(data):
    c = 0xFFFFFFFF
    for b in data:
        c ^= b << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if c & 0x80000000 else (c << 1) & 0xFFFFFFFF
    return c ^ 0xFFFFFFFF


def _stored_block_crcs(data):
    """(block CRCs, stream CRC) of a one-stream file written by Python's bz2: block magics found by a bit scan"""
    x = int.from_bytes(data, "big")
    n = len(data) * 8
    starts = []
    for s in range(8):                         # the magic's bytes in the file shifted left by s bits
        y = (x << s).to_bytes(len(data) + 1, "big")
        i = y.find(b"\x31\x41\x59\x26\x53\x59")
        while i >= 0:
            starts.append(8 * i - 8 + s)
            i = y.find(b"\x31\x41\x59\x26\x53\x59", i + 1)
    crcs = [(x >> (n - bit - 80)) & 0xFFFFFFFF for bit in sorted(starts)]
    for pad in range(8):
        if (x >> (pad + 32)) & ((1 << 48) - 1) == 0x177245385090:
            return crcs, (x >> pad) & 0xFFFFFFFF
    raise AssertionError("no end-of-stream magic")


def test_crc_pieces_against_bitwise_crc_and_stored_crcs(plan):
    rng = np.random.default_rng(9)
    for n in (0, 1, 7, 4096, 4097, 100_000):
        data = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        want = _bitwise_crc(data)
        assert plan.bp_crc_raw(data, n, 0xFFFFFFFF) ^ 0xFFFFFFFF == want
        for piece in (1, 3, 64, 4096, 1 << 20):
            assert plan.bp_crc_pieces(data, n, piece) == want, (n, piece)
    # a one-block stream: its block CRC is the CRC of the text, and the stream CRC rotl-combines the block CRCs
    text = fastq_text(rng, 500)
    crcs, stream = _stored_block_crcs(bz2.compress(text, 9))
    assert crcs == [_bitwise_crc(text)] and plan.bp_crc_pieces(text, len(text), 4096) == crcs[0]
    text = fastq_text(rng, 4000, quals="const") * 2
    crcs, stream = _stored_block_crcs(bz2.compress(text, 1))
    assert len(crcs) >= 3
    arr = (C.c_uint32 * len(crcs))(*crcs)
    assert plan.bp_combine(arr, len(crcs)) == stream


def chain(plan, files, extra=(), batch=1000):
    bufs = (C.c_char_p * len(files))(*files)
    sizes = (C.c_uint64 * len(files))(*[len(f) for f in files])
    ex = (C.c_uint64 * max(1, len(extra)))(*extra)
    info = (C.c_uint64 * 3)()
    cap = 4096
    crcs, ns, fo = (C.c_uint32 * cap)(), (C.c_uint32 * cap)(), (C.c_uint32 * cap)()
    err = C.create_string_buffer(256)
    rc = plan.bp_model_chain(bufs, sizes, len(files), ex, len(extra), batch, info, crcs, ns, fo, cap, err, 256)
    if rc:
        return None, err.value.decode()
    nb = int(info[1])
    return dict(streams=int(info[0]), blocks=nb, candidates=int(info[2]), crcs=list(crcs[:nb]), ns=list(ns[:nb]), files=list(fo[:nb])), ""


def test_chain_walk_with_false_candidates_and_streams(plan):
    rng = np.random.default_rng(10)
    a, b = fastq_text(rng, 3000), fastq_text(rng, 2000, quals="const")
    one = bz2.compress(a, 1)
    crcs, _ = _stored_block_crcs(one)
    for extra in ((), (33, 100, 1000, len(one) * 8 - 200), tuple(int(x) for x in rng.integers(40, len(one) * 8 - 100, size=50))):
        for batch in (1, 3, 1000):
            got, why = chain(plan, [one], extra, batch)
            assert got, why
            assert got["streams"] == 1 and got["crcs"] == crcs and sum(got["ns"]) > 0, (extra, batch)
    # several streams (pbzip2's layout), an empty one among them, and two files in one call
    multi = bz2.compress(a, 1) + bz2.compress(b"", 9) + bz2.compress(b, 3)
    got, why = chain(plan, [multi, one], (77, 5000), 2)
    assert got, why
    assert got["streams"] == 4 and got["files"].count(1) == len(crcs)
    assert got["crcs"][-len(crcs):] == crcs


def test_chain_walk_declines(plan):
    rng = np.random.default_rng(11)
    good = bz2.compress(fastq_text(rng, 3000), 9)
    for name, data in {"trailing": good + b"garbage!", "truncated": good[:-4], "header": b"BZh0" + good[4:], "empty": b""}.items():
        got, why = chain(plan, [data])
        assert got is None and why, name
    stream_crc = bytearray(good)
    stream_crc[-2] ^= 0x40                     # inside the stream CRC or its padding: the CRC must differ, or the padding is ignored
    got, why = chain(plan, [bytes(stream_crc)])
    assert (got is None and "combined CRC" in why) or got is not None
    rnd = bytearray(good)
    rnd[14] |= 0x80                            # the randomised bit of the first block
    got, why = chain(plan, [bytes(rnd)])
    assert got is None and "randomised" in why


def test_run_length_scan_matches_straight_decode(plan):
    rng = np.random.default_rng(12)
    for trial in range(40):
        # an RLE1 text as bzip2 writes it: runs of 4 equal bytes are followed by a count
        parts = []
        for _ in range(int(rng.integers(1, 400))):
            c = bytes([int(rng.choice([65, 67, 71, 84, 0, 255]))])
            r = int(rng.choice([1, 2, 3, 4]))
            parts.append(c * r + (bytes([int(rng.integers(0, 256))]) if r == 4 else b""))
        pre = b"".join(parts)
        # (two neighbouring parts of the same byte would form a longer run: the check compares both decodes anyway)
        out = C.create_string_buffer(len(pre) * 260 + 16)
        straight = plan.bp_rle_check(pre, len(pre), len(pre) + 1, out, len(pre) * 260 + 16)
        for chunk in (1, 2, 3, 5, 7, 64, 256):
            assert plan.bp_rle_check(pre, len(pre), chunk, out, len(pre) * 260 + 16) == straight, (trial, chunk)
    assert plan.bp_rle_check(b"AAAA", 4, 2, C.create_string_buffer(16), 16) == -2          # a count due at the end: declined
    assert plan.bp_rle_check(b"AAAA\x05B", 6, 1, C.create_string_buffer(64), 64) == 10
