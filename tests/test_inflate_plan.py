"""CPU tests of the device inflate's bookkeeping (sylph_amd/csrc/inflate_plan.h, the very header csrc/inflate.hip includes): CRC-32 put
together from shifted pieces, gzip member headers, and the chain walk — driven by a CPU model of the device kernels' reports
(tests/inflate_plan_capi.cpp) and checked against zlib.  The GPU kernels themselves are tested in tests/test_gpu_inflate.py."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from .helpers import bgzf_compress, build_path, golden_bytes

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def L():
    src = os.path.join(HERE, "inflate_plan_capi.cpp")
    out, stale = build_path("sylph_inflate_plan", [src] + [os.path.join(HERE, "..", "sylph_amd", "csrc", h) for h in ("inflate_plan.h", "stream_plan.h")], ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, src, "-lz"])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    lib.ip_member_body.restype = C.c_uint64
    lib.ip_member_body.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64]
    lib.ip_crc_members.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32)]
    lib.ip_crc_shift.restype = C.c_uint32
    lib.ip_crc_shift.argtypes = [C.c_uint32, C.c_uint64]
    lib.ip_model_inflate.restype = C.c_longlong
    lib.ip_model_inflate.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    lib.ip_region_ratio.restype = C.c_uint64
    lib.ip_region_ratio.argtypes = [C.POINTER(C.c_char_p), u64p, C.c_uint32, C.c_uint64]
    lib.ip_decode_job.argtypes = [C.c_uint32, u64p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, u64p]
    lib.ip_cells_layout.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, u64p]
    lib.ip_window_group.restype = C.c_uint32
    lib.ip_window_group.argtypes = [C.c_uint32]
    lib.ip_redo_plan.restype = C.c_uint64
    lib.ip_redo_plan.argtypes = [u32p, u32p, C.c_uint32, u64p, u32p, u64p, u32p]
    return lib


def model(L, gz, cap, ratio=16, slack=1024):
    out = C.create_string_buffer(max(cap, 1))
    info = (C.c_uint64 * 5)()
    err = C.create_string_buffer(256)
    n = L.ip_model_inflate(gz, len(gz), out, cap, info, ratio, slack, err, 256)
    if n < 0:
        return None, err.value.decode(), None
    return out.raw[:n], "", dict(members=info[0], blocks=info[1], candidates=info[2], host_members=info[3], redone=info[4])


def gz_level(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, 31, 8, strategy)
    return co.compress(data) + co.flush()


def fastq_text(rng, n):
    out = []
    for i in range(n):
        L_ = int(rng.integers(50, 200))
        out.append(b"@read%d/1\n" % i + rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=L_).tobytes() + b"\n+\n" +
                   np.repeat(rng.choice(np.frombuffer(b"F:,#", dtype=np.uint8), size=L_ // 5 + 1), 5)[:L_].tobytes() + b"\n")
    return b"".join(out)


def test_crc_from_shifted_pieces_equals_zlib(L):
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, size=300001, dtype=np.uint8).tobytes()
    for ends in ([len(data)], [1, 2, 1500, 1500, 70000, len(data)], [0, 0, len(data)], list(range(1000, len(data), 9973)) + [len(data)]):
        for piece in (1024, 4096, 7):
            if piece == 7 and len(ends) > 3:
                continue
            e = (C.c_uint64 * len(ends))(*ends)
            out = (C.c_uint32 * len(ends))()
            L.ip_crc_members(data, len(data), piece, e, len(ends), out)
            begin = 0
            for i, z in enumerate(ends):
                assert out[i] == zlib.crc32(data[begin:z]), (ends[:4], piece, i)
                begin = z
    # the register after n zero bytes
    for n in (0, 1, 5, 1 << 20, (1 << 33) + 12345):
        want = 0x12345678
        if n <= 1 << 20:
            tab = [0] * 256
            for i in range(256):
                c = i
                for _ in range(8):
                    c = (c >> 1) ^ 0xEDB88320 if c & 1 else c >> 1
                tab[i] = c
            for _ in range(n):
                want = tab[want & 0xFF] ^ (want >> 8)
            assert L.ip_crc_shift(0x12345678, n) == want
        else:   # composition
            assert L.ip_crc_shift(0x12345678, n) == L.ip_crc_shift(L.ip_crc_shift(0x12345678, 1 << 33), 12345)


def test_member_headers(L):
    plain = gzip.compress(b"hello")
    assert L.ip_member_body(plain, len(plain), 0) == 10
    hdr = b"\x1f\x8b\x08" + bytes([4 | 8 | 16 | 2]) + b"\0\0\0\0\0\xff" + struct.pack("<H", 5) + b"extra" + b"name.fq\0" + b"a comment\0" + b"\x12\x34"
    whole = hdr + plain[10:]
    assert L.ip_member_body(whole, len(whole), 0) == len(hdr)
    assert L.ip_member_body(b"\x1f\x8b\x07" + plain[3:], len(plain), 0) == 0         # not deflate
    assert L.ip_member_body(plain[:12], 12, 0) == 0                                 # too short to hold a trailer
    assert L.ip_member_body(b"@read\nACGT\n+\nIIII\n" * 4, 64, 0) == 0
    b = bgzf_compress(b"ACGT" * 100)
    assert L.ip_member_body(b, len(b), 0) == 18


@pytest.mark.parametrize("level", [1, 6, 9])
def test_model_road_equals_zlib(L, level):
    text = fastq_text(np.random.default_rng(level), 12000)
    got, why, info = model(L, gz_level(text, level), len(text) + 16)
    assert why == "" and got == text
    assert info["members"] == 1 and info["blocks"] >= 4 and info["candidates"] <= info["blocks"] + 1


def test_model_road_members_bgzf_stored_fixed(L):
    rng = np.random.default_rng(4)
    a, b, c = fastq_text(rng, 3000), fastq_text(rng, 5), fastq_text(rng, 4000)
    got, why, info = model(L, gz_level(a, 6) + gz_level(b, 6) + gz_level(b"", 6) + gz_level(c, 1), len(a + b + c) + 16)
    assert why == "" and got == a + b + c and info["members"] == 4 and info["host_members"] >= 1
    text = a + c
    got, why, info = model(L, bgzf_compress(text), len(text) + 16)
    assert why == "" and got == text and info["members"] == len(range(0, len(text), 65280)) + 1
    noise = rng.integers(0, 256, size=100000, dtype=np.uint8).tobytes()
    for gz in (gz_level(noise, 0), gz_level(noise, 6), gz_level(b"ACGT" * 5, 6), gz_level(b"", 6), gz_level(a, 6, zlib.Z_FIXED)):
        want = gzip.decompress(gz)
        got, why, info = model(L, gz, len(want) + 16)
        assert why == "" and got == want
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    parts = [co.compress(a[i:i + 7001]) + co.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(a), 7001)]
    got, why, info = model(L, b"".join(parts) + co.flush(), len(a) + 16)
    assert why == "" and got == a


def test_model_road_declines_damage(L):
    text = fastq_text(np.random.default_rng(6), 6000)
    gz = gz_level(text, 6)
    cap = len(text) + 16
    assert model(L, text[:5000], cap)[0] is None
    assert model(L, gz[: len(gz) // 2], cap)[0] is None
    assert model(L, gz[:-1], cap)[0] is None
    assert model(L, gz + b"garbage", cap)[0] is None
    for at, bit in ((len(gz) // 2, 0x10), (len(gz) - 8, 1), (len(gz) - 1, 1)):
        bad = bytearray(gz)
        bad[at] ^= bit
        assert model(L, bytes(bad), cap)[0] is None, at
    # a region too small for its block (here: a ratio no FASTQ block meets) is not damage: the block is decoded again with room for it
    got, why, info = model(L, gz, cap, ratio=1, slack=0)
    assert why == "" and got == text and info["redone"] == info["blocks"] >= 2
    got, why, info = model(L, gz, cap)
    assert got == text and info["redone"] == 0


def test_reference_fasta_gz_through_the_model(L):
    gz = golden_bytes(os.path.join("ref_test_files", "e.coli-K12.fasta.gz"))
    want = gzip.decompress(gz)
    # the model tests every bit position one bit at a time: cut the file's text to 600 kB and re-deflate it the way the file was (zlib level 6)
    cut = want[:600000]
    got, why, info = model(L, gz_level(cut, 6), len(cut) + 16)
    assert why == "" and got == cut and info["blocks"] >= 3


# ---- where the cells go (inflate_plan.h: region_ratio_from_isize, decode_job, cells_layout, redo_plan, window_group), against the rules
# restated here

SLACK, SPILL_SLOTS, SPILL_CELLS = 1024, 96, 1 << 20


def decode_jobs(L, cand, body0, byte_end, ratio, slack=SLACK):
    c = (C.c_uint64 * len(cand))(*cand)
    out = (C.c_uint64 * 4)()
    jobs = []
    for i in range(len(cand)):
        L.ip_decode_job(i, c, len(cand), body0, byte_end, ratio, slack, out)
        jobs.append(tuple(out))
    return jobs


@pytest.mark.parametrize("ratio", [1, 9, 16])
def test_candidate_regions_follow_the_rule_and_never_overlap(L, ratio):
    body0, n = 10, 5000
    cand = [8 * body0, 8 * body0 + 3, 8 * (body0 + 1), 8 * (n - 1) + 7]
    jobs = decode_jobs(L, cand, body0, n, ratio)
    for i, (start, region, cap, have_window) in enumerate(jobs):
        b0, b1 = cand[i] // 8, (cand[i + 1] // 8 if i + 1 < len(cand) else n)
        assert start == cand[i] and have_window == (i != 0)
        assert region == (b0 - body0) * ratio + i * SLACK
        assert cap == min(0xFFFFFF00, (b1 - b0) * ratio + SLACK)
    for (_, region, cap, _), (_, next_region, _, _) in zip(jobs, jobs[1:]):
        assert region + cap <= next_region
    out = (C.c_uint64 * 3)()
    L.ip_cells_layout(n - body0, len(cand), ratio, SLACK, SPILL_SLOTS, SPILL_CELLS, out)
    n_cells, spill_base, total = out
    assert n_cells == (n - body0) * ratio + len(cand) * SLACK + 64 and jobs[-1][1] + jobs[-1][2] <= n_cells
    assert spill_base == (n_cells + 63) // 64 * 64 and total == spill_base + SPILL_SLOTS * SPILL_CELLS + 64


def test_a_region_holds_no_more_cells_than_a_block_may_have(L):
    body0 = 10
    cand = [8 * body0, 8 * (body0 + (1 << 28))]
    jobs = decode_jobs(L, cand, body0, body0 + (1 << 28) + 100, 16)
    assert (1 << 28) * 16 + SLACK > 0xFFFFFF00 and jobs[0][2] == 0xFFFFFF00
    assert jobs[1][1] == (1 << 28) * 16 + SLACK and jobs[1][2] == 100 * 16 + SLACK


def region_ratio(L, files, flat):
    ptrs = (C.c_char_p * len(files))(*files)
    sizes = (C.c_uint64 * len(files))(*[len(f) for f in files])
    return L.ip_region_ratio(ptrs, sizes, len(files), flat)


def test_region_ratio_from_isize(L):
    def file_of(n_bytes, isize):
        return b"\x1f\x8b\x08" + b"\xAA" * (n_bytes - 7) + struct.pack("<I", isize)
    for flat in (16, 100):
        for isize, want in ((1490, flat), (1500, 4), (5300, 9), (40000, 62), (40010, flat)):       # r = 1.49, 1.5, 5.3, 40, 40.01 of 1000 bytes
            r = isize / 1000
            assert want == (flat if r < 1.5 or r > 40 else int(r * 1.5) + 2)
            assert region_ratio(L, [file_of(1000, isize)], flat) == min(flat, want), (flat, isize)
        assert region_ratio(L, [file_of(1000, 5300), file_of(500, 4000)], flat) == min(flat, 14)    # the worst file: r = 8
        assert region_ratio(L, [file_of(1000, 5300), file_of(1000, 1000)], flat) == flat            # one file out of range
        assert region_ratio(L, [file_of(1000, 50000), file_of(1000, 5300)], flat) == flat


def test_window_group(L):
    for KB, want in ((1, 8), (63, 8), (64, 8), (65, 9), (10000, 100)):
        G = L.ip_window_group(KB)
        assert G == want and G >= 8 and G * G >= KB and (G == 8 or (G - 1) * (G - 1) < KB)


def test_blocks_decoded_again_are_packed_at_multiples_of_64_cells(L):
    n_out = [1, 5000, 63, 64, 7, 65, 1]
    flags = [2, 1, 2, 3, 0, 2, 2]
    KB = len(n_out)
    region, cap, start, win = (C.c_uint64 * KB)(), (C.c_uint32 * KB)(), (C.c_uint64 * KB)(), (C.c_uint32 * KB)()
    cells = L.ip_redo_plan((C.c_uint32 * KB)(*n_out), (C.c_uint32 * KB)(*flags), KB, region, cap, start, win)
    at = 0
    for i in range(KB):
        if not flags[i] & 2:
            assert region[i] == 0xFFFFFFFFFFFFFFFF
            continue
        assert region[i] == at and at % 64 == 0 and cap[i] == n_out[i] and start[i] == 100 + i and win[i] == (i != 0)
        at += (n_out[i] + 63) // 64 * 64
    assert cells == at == 64 + 64 + 64 + 128 + 64
