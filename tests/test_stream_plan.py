"""CPU tests of what the two device decompressors' plan headers share (sylph_amd/csrc/stream_plan.h, compiled with g++ through
tests/stream_plan_capi.cpp): CRC-32 in both bit orders put together from shifted pieces, against zlib.crc32 and a bitwise MSB-first
loop written here; shifts against a square-and-multiply written here; Segments::find.  And the headers' stand-alone sanitizer run."""
import bz2
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

from .helpers import build_path

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "sylph_amd", "csrc")


@pytest.fixture(scope="module")
def L():
    src = os.path.join(HERE, "stream_plan_capi.cpp")
    out, stale = build_path("sylph_stream_plan", [src, os.path.join(CSRC, "stream_plan.h")], ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, src])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    lib.sp_crc_pieces.restype = C.c_uint32
    lib.sp_crc_pieces.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.c_uint64]
    lib.sp_crc_shift.restype = C.c_uint32
    lib.sp_crc_shift.argtypes = [C.c_int, C.c_uint32, C.c_uint64]
    lib.sp_segments_find.restype = C.c_uint64
    lib.sp_segments_find.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.sp_one_segment_total.restype = C.c_uint64
    lib.sp_one_segment_total.argtypes = [C.c_char_p, C.c_uint64]
    return lib


def crc32_bzip2(data):
    """CRC-32/BZIP2 one bit at a time: polynomial 0x04C11DB7, MSB first, initial value and final XOR 0xFFFFFFFF"""
    reg = 0xFFFFFFFF
    for byte in data:
        reg ^= byte << 24
        for _ in range(8):
            reg = ((reg << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if reg & 0x80000000 else (reg << 1) & 0xFFFFFFFF
    return reg ^ 0xFFFFFFFF


def polymulmod(a, b):
    """a * b mod x^32 + 0x04C11DB7 over GF(2); bit i of an int is the coefficient of x^i"""
    p = 0
    while b:
        if b & 1:
            p ^= a
        b >>= 1
        a <<= 1
        if a >> 32:
            a ^= 0x104C11DB7
    return p


def shifted(reg, n_bytes, reflected):
    """the CRC loop's register after n_bytes zero bytes: reg * x^(8 n) mod P, by square and multiply"""
    rev = lambda v: int(f"{v:032b}"[::-1], 2)
    acc, sq, e = (rev(reg) if reflected else reg), 2, 8 * n_bytes
    while e:
        if e & 1:
            acc = polymulmod(acc, sq)
        sq = polymulmod(sq, sq)
        e >>= 1
    return rev(acc) if reflected else acc


@pytest.mark.parametrize("reflected", [1, 0])
def test_crc_from_pieces_equals_an_independent_crc(L, reflected):
    data = np.random.default_rng(7).integers(0, 256, size=4097, dtype=np.uint8).tobytes()
    for n in (0, 1, 3, 4, 63, 64, 65, 4097):
        want = zlib.crc32(data[:n]) if reflected else crc32_bzip2(data[:n])
        for piece in (1, 7, 64):
            assert L.sp_crc_pieces(reflected, data, n, piece) == want, (n, piece)
    assert crc32_bzip2(b"123456789") == 0xFC891918 and zlib.crc32(b"123456789") == 0xCBF43926      # the catalogued check values


@pytest.mark.parametrize("reflected", [1, 0])
def test_crc_shift(L, reflected):
    for reg in (0x12345678, 0xFFFFFFFF, 1, 0x80000000, 0):
        assert L.sp_crc_shift(reflected, reg, 0) == reg
        for n in (1, 5, (1 << 32) + 5):
            assert L.sp_crc_shift(reflected, reg, n) == shifted(reg, n, reflected), (hex(reg), n)
    # the square-and-multiply itself, against the byte loop: a register run through 5 zero bytes
    reg = 0x12345678
    for _ in range(5 * 8):
        reg = (reg >> 1) ^ 0xEDB88320 if reg & 1 else reg >> 1
    assert shifted(0x12345678, 5, 1) == reg


def test_segments_find(L):
    sizes = (C.c_uint64 * 3)(1, 18, 5)
    total = C.c_uint64(0)
    for pos, want in ((0, 0), (1, 1), (18, 1), (19, 2), (23, 2)):          # every file's first and last byte
        assert L.sp_segments_find(sizes, 3, pos, C.byref(total)) == want, pos
        assert total.value == 24
    assert L.sp_one_segment_total(b"abc", 3) == 3


def test_standalone_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/stream_sanitize_main.cpp + the three *_plan_capi.cpp models, built with AddressSanitizer and UBSan into a program of its own
    and run on the CPU over a small multi-member gzip file and a two-stream bzip2 file: nothing is loaded into this interpreter."""
    srcs = [os.path.join(HERE, f) for f in ("stream_sanitize_main.cpp", "stream_plan_capi.cpp", "inflate_plan_capi.cpp", "bunzip2_plan_capi.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("stream_plan.h", "inflate_plan.h", "bunzip2_plan.h")]
    exe, stale = build_path("sylph_stream_sanitize", deps)
    if stale:
        tmp = exe + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                               "-Werror", "-o", tmp] + srcs + ["-lz"])
        os.replace(tmp, exe)
    rng = np.random.default_rng(3)
    recs = [b"@read%d/1\n" % i + rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.integers(50, 200))).tobytes() + b"\n+\nFFFF:,#\n" for i in range(60)]
    a, b = b"".join(recs[:56]), b"".join(recs[56:])

    def member(d):
        co = zlib.compressobj(6, zlib.DEFLATED, 31)
        return co.compress(d) + co.flush()
    co = zlib.compressobj(6, zlib.DEFLATED, 31)               # two blocks in the first member, then a small member and an empty one
    first = co.compress(a[: len(a) // 2]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(a[len(a) // 2:]) + co.flush()
    (tmp_path / "m.gz").write_bytes(first + member(b) + member(b""))
    (tmp_path / "m.txt").write_bytes(a + b)
    (tmp_path / "m.bz2").write_bytes(bz2.compress(a, 1) + bz2.compress(b, 9))
    p = subprocess.run([exe] + [str(tmp_path / f) for f in ("m.gz", "m.txt", "m.bz2")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "stream sanitize run ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
