"""CPU tests of the streamed device inflate's bookkeeping (sylph_amd/csrc/inflate_stream_plan.h, the header csrc/inflate.hip's stream
includes): the cut, the carry, the resumable chain walk and the CRC continued across slices — driven one slice at a time by the CPU
model of the device kernels (tests/inflate_stream_plan_capi.cpp, which includes the model of tests/inflate_plan_capi.cpp) and checked
against zlib.  The GPU side is tested in tests/test_gpu_inflate_stream.py."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from .helpers import bgzf_compress, build_path
from .test_inflate_plan import fastq_text, gz_level

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "sylph_amd", "csrc")
SRCS = [os.path.join(HERE, f) for f in ("inflate_stream_plan_capi.cpp", "inflate_plan_capi.cpp")]
HEADERS = [os.path.join(CSRC, h) for h in ("inflate_stream_plan.h", "inflate_plan.h", "stream_plan.h")]
KiB = 1024
TRACE = 12


@pytest.fixture(scope="module")
def L():
    out, stale = build_path("sylph_inflate_stream_plan", SRCS + HEADERS, ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, SRCS[0], "-lz"])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    lib.isp_slice_cut.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, u64p]
    lib.isp_overlap.restype = C.c_uint64
    lib.isp_overlap.argtypes = [C.c_uint64]
    lib.isp_max_grow.restype = C.c_uint32
    lib.isp_whole_chain.restype = C.c_longlong
    lib.isp_whole_chain.argtypes = [C.c_char_p, C.c_uint64, u64p, u64p, C.c_uint32, u32p]
    lib.isp_model_stream.restype = C.c_longlong
    lib.isp_model_stream.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64, u64p, C.c_uint32, u32p, u64p, C.c_uint32,
                                     u32p, u64p, C.c_char_p, C.c_size_t]
    return lib


class Run:
    pass


def stream(L, gz, slice_bytes, cap, ratio=16, slack=1024):
    """the sliced model road -> Run: .text (None: declined, .why), .good = the text of the slices before the failing one, .slices = one
    dict per slice, .blocks = the chain blocks' start bits in the order they were decoded into the text"""
    out = C.create_string_buffer(max(cap, 1))
    trace = (C.c_uint64 * (TRACE * 4096))()
    blocks = (C.c_uint64 * 65536)()
    ns, nb, good = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    err = C.create_string_buffer(256)
    n = L.isp_model_stream(gz, len(gz), slice_bytes, ratio, slack, out, cap, trace, 4096, C.byref(ns), blocks, 65536, C.byref(nb), C.byref(good), err, 256)
    r = Run()
    r.text = out.raw[:n] if n >= 0 else None
    r.why = err.value.decode()
    r.good = out.raw[:good.value]
    names = ("pos", "cut", "end", "in_bit", "in_member", "in_len", "out_bit", "out_member", "out_len", "new_bytes", "grown", "spanning")
    r.slices = [dict(zip(names, trace[i * TRACE:(i + 1) * TRACE])) for i in range(ns.value)]
    r.blocks = list(blocks[:nb.value])
    return r


def whole_chain(L, gz):
    b, m = (C.c_uint64 * 65536)(), (C.c_uint64 * 65536)()
    nm = C.c_uint32(0)
    nb = L.isp_whole_chain(gz, len(gz), b, m, 65536, C.byref(nm))
    assert nb >= 0
    return list(b[:nb]), list(m[:nm.value])


@pytest.fixture(scope="module")
def text3mb():
    return {level: fastq_text(np.random.default_rng(level), 12000) for level in (1, 6, 9)}          # 3.19 MB: 35, 25 and 22 deflate blocks


@pytest.mark.parametrize("slice_kib", [64, 128, 256])
@pytest.mark.parametrize("level", [1, 6, 9])
def test_sliced_model_road_equals_zlib_and_keeps_the_cut_rule(L, text3mb, level, slice_kib):
    text = text3mb[level]
    gz = gz_level(text, level)
    r = stream(L, gz, slice_kib * KiB, len(text) + 16)
    assert r.why == "" and r.text == text == zlib.decompress(gz, 31)
    assert len(r.slices) > 1
    block_bits, member_ends = whole_chain(L, gz)
    # no block is decoded into the text twice, none is left out, and they come in the chain's order
    assert r.blocks == block_bits
    entry = dict(in_bit=0, in_member=0, in_len=0)
    done = 0
    for j, s in enumerate(r.slices):
        # the carry of slice j is the entry state of slice j + 1
        assert (s["in_bit"], s["in_member"], s["in_len"]) == (entry["in_bit"], entry["in_member"], entry["in_len"]), j
        assert s["pos"] == s["in_bit"] // 8 and s["cut"] == min(len(gz), s["pos"] + (slice_kib * KiB << s["grown"]))
        assert s["end"] == min(len(gz), s["cut"] + L.isp_overlap(slice_kib * KiB << s["grown"]))
        # every slice ends on a chain block's start or behind a member's trailer, in front of the first block at or behind the cut
        if s["out_member"]:
            assert s["out_bit"] in block_bits
            assert s["out_bit"] // 8 >= s["cut"] or s["end"] < len(gz)
        else:
            assert s["out_bit"] in member_ends
        inside = [b for b in block_bits if s["in_bit"] <= b < s["out_bit"]]
        assert inside and all(b // 8 < s["cut"] for b in inside)
        done += s["new_bytes"]
        assert s["out_len"] == (done if s["out_member"] else 0)                 # one member: its length so far is the text so far
        entry = dict(in_bit=s["out_bit"], in_member=s["out_member"], in_len=s["out_len"])
    assert done == len(text) and r.slices[-1]["out_bit"] == len(gz) * 8


def test_slice_cut_arithmetic(L):
    out = (C.c_uint64 * 3)()
    for bit, n, sl in ((0, 10 ** 6, 64 * KiB), (8 * 70000 + 3, 10 ** 6, 128 * KiB), (8 * 999000, 10 ** 6, 64 * KiB), (0, 1000, 64 * KiB), (0, 10 ** 9, 64 << 20)):
        L.isp_slice_cut(bit, n, sl, out)
        ov = L.isp_overlap(sl)
        assert ov == min(max(sl // 2, 32 * KiB), 1 << 20)
        assert tuple(out) == (bit // 8, min(n, bit // 8 + sl), min(n, bit // 8 + sl + ov))


def crossing_text(rng):
    """(text, first, second): text[first:second] is 30 kB of noise and text[second:second + 30000] repeats it — deflate writes the repeat as
    matches at distance 30000 (under 32 KiB), and a block of literals holds 16 Ki symbols at most, so a block starts inside the first copy"""
    half = rng.integers(0, 256, size=30000, dtype=np.uint8).tobytes()
    head = fastq_text(rng, 1100)
    return head + half + half + fastq_text(rng, 300), len(head), len(head) + len(half)


def test_a_back_reference_crosses_the_cut(L):
    text, first, second = crossing_text(np.random.default_rng(11))
    gz = gz_level(text, 6)
    block_bits, _ = whole_chain(L, gz)
    crossed = 0
    for b in block_bits:
        if b // 8 < 64 * KiB:
            continue
        r = stream(L, gz, b // 8, len(text) + 16)           # the first slice ends in front of the block at bit b
        assert r.why == "" and r.text == text and r.slices[0]["out_bit"] == b
        at = r.slices[0]["new_bytes"]
        if at > second:
            break
        crossed += first < at <= second                     # the cut lies inside the first copy: every match of the second reaches over it
    assert crossed >= 1


def members(parts, level=6):
    return b"".join(gz_level(p, level) for p in parts)


@pytest.mark.parametrize("delta", [0, -1, 1])
def test_member_boundary_on_before_and_behind_a_slice_end(L, delta):
    rng = np.random.default_rng(12)
    a, b = fastq_text(rng, 2600), fastq_text(rng, 2000)
    ga, gb = gz_level(a, 6), gz_level(b, 6)
    # slice 0 ends exactly `delta` bytes from the first member's end: the slice size is chosen for it (the minimum is 64 KiB)
    slice_bytes = len(ga) - delta
    assert slice_bytes >= 64 * KiB
    r = stream(L, ga + gb, slice_bytes, len(a + b) + 16)
    assert r.why == "" and r.text == a + b and len(r.slices) >= 2
    assert r.slices[0]["cut"] == len(ga) - delta
    assert not r.slices[0]["out_member"] and r.slices[0]["out_bit"] == len(ga) * 8


def test_bgzf_with_its_empty_final_member(L):
    rng = np.random.default_rng(13)
    text = fastq_text(rng, 3000)
    gz = bgzf_compress(text)
    r = stream(L, gz, 64 * KiB, len(text) + 16)
    assert r.why == "" and r.text == text and len(r.slices) >= 3
    assert all(not s["out_member"] or s["out_bit"] // 8 >= s["cut"] or s["end"] < len(gz) for s in r.slices)
    _, member_ends = whole_chain(L, gz)
    assert len(member_ends) == len(range(0, len(text), 65280)) + 1


def test_a_member_that_spans_three_slices_has_its_crc_continued(L):
    rng = np.random.default_rng(14)
    a, b, c = fastq_text(rng, 200), fastq_text(rng, 3200), fastq_text(rng, 200)
    gz = members([a, b, c])
    r = stream(L, gz, 64 * KiB, len(a + b + c) + 16)
    assert r.why == "" and r.text == a + b + c
    inside = [s for s in r.slices if s["in_member"]]
    assert len(inside) >= 2 and sum(s["spanning"] for s in r.slices) == 1          # entered twice inside the member: three slices; checked once, where it ends
    # the continued register is what the check used: a wrong CRC in that member's trailer is found in the slice where it ends
    end_b = len(gz_level(a, 6)) + len(gz_level(b, 6))
    bad = bytearray(gz)
    bad[end_b - 8] ^= 1
    r2 = stream(L, bytes(bad), 64 * KiB, len(a + b + c) + 16)
    assert r2.text is None and "CRC" in r2.why and r2.good == (a + b)[:len(r2.good)] and len(r2.good) >= len(a)


def test_a_first_block_larger_than_the_slice_doubles_it(L):
    rng = np.random.default_rng(15)
    noise = rng.integers(0, 256, size=300000, dtype=np.uint8).tobytes()       # stored blocks: ONE chain block of 300 KB behind the first header
    a, c = fastq_text(rng, 1200), fastq_text(rng, 1200)
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    gz = co.compress(a) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(noise) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(c) + co.flush()
    text = a + noise + c
    r = stream(L, gz, 64 * KiB, len(text) + 16)
    assert r.why == "" and r.text == text
    assert max(s["grown"] for s in r.slices) >= 2                              # 64 + 32 KiB, 128 + 64 KiB do not hold it; 256 + 128 KiB do
    assert r.slices[0]["grown"] == 0


def test_a_block_that_never_fits_within_the_retry_bound_declines(L):
    rng = np.random.default_rng(16)
    n_noise = (64 * KiB << L.isp_max_grow()) + (1 << 20) + 200000               # more than the slice doubled as often as it may be, + its overlap
    noise = rng.integers(0, 256, size=n_noise, dtype=np.uint8).tobytes()
    a = fastq_text(rng, 1200)
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    gz = co.compress(a) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(noise) + co.flush()
    r = stream(L, gz, 64 * KiB, len(a) + n_noise + 16)
    assert r.text is None and "does not fit the slice" in r.why
    assert r.good == a[:len(r.good)]


@pytest.fixture(scope="module")
def damaged():
    text = fastq_text(np.random.default_rng(17), 6000)                          # 1.6 MB: 400 KB of gzip, seven slices of 64 KiB
    return text, gz_level(text, 6)


def check_declined(r, text, at_least=0):
    assert r.text is None and r.why
    assert r.good == text[:len(r.good)] and len(r.good) >= at_least              # what the earlier slices gave was right


def test_damage_a_flipped_bit_in_the_third_slice(L, damaged):
    text, gz = damaged
    good = stream(L, gz, 64 * KiB, len(text) + 16)
    assert good.text == text and len(good.slices) >= 5
    s2 = good.slices[2]
    # (a flipped bit among a block's symbols may only change a literal, which nothing but the member's CRC can see, at the member's end;
    #  the bit flipped here is the low BTYPE bit of the slice's second block: 2 = dynamic becomes 3 = invalid, and the chain breaks there)
    inside = [b for b in good.blocks if s2["in_bit"] <= b < s2["out_bit"]]
    assert len(inside) >= 2
    bad = bytearray(gz)
    bad[(inside[1] + 1) // 8] ^= 1 << ((inside[1] + 1) % 8)
    r = stream(L, bytes(bad), 64 * KiB, len(text) + 16)
    check_declined(r, text, at_least=good.slices[0]["new_bytes"] + good.slices[1]["new_bytes"])
    assert len(r.good) < sum(s["new_bytes"] for s in good.slices[:3])            # declined at the slice that holds it, not later


def test_damage_crc_isize_truncation_and_trailing_garbage(L, damaged):
    text, gz = damaged
    cap = len(text) + 16
    before_last = sum(s["new_bytes"] for s in stream(L, gz, 64 * KiB, cap).slices[:-1])
    crc = bytearray(gz); crc[-8] ^= 1
    isize = bytearray(gz); isize[-1] ^= 1
    for bad in (bytes(crc), bytes(isize), gz + b"garbage", gz[:-1], gz[:-9]):
        check_declined(stream(L, bad, 64 * KiB, cap), text, at_least=before_last)
    check_declined(stream(L, gz[:len(gz) // 2], 64 * KiB, cap), text, at_least=1)
    check_declined(stream(L, text[:5000], 64 * KiB, cap), text)


def test_regions_too_small_are_decoded_again_in_every_slice(L, damaged):
    text, gz = damaged
    r = stream(L, gz, 64 * KiB, len(text) + 16, ratio=1, slack=0)
    assert r.why == "" and r.text == text


def test_standalone_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/inflate_stream_sanitize_main.cpp + the model, built with AddressSanitizer and UBSan into a program of its own and run as a
    child process over the inputs of the tests above: host code only, nothing is loaded into this interpreter."""
    main = os.path.join(HERE, "inflate_stream_sanitize_main.cpp")
    exe, stale = build_path("sylph_inflate_stream_sanitize", [main] + SRCS + HEADERS)
    if stale:
        tmp = exe + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                               "-o", tmp, main, SRCS[0], "-lz"])
        os.replace(tmp, exe)
    rng = np.random.default_rng(18)
    a, b = fastq_text(rng, 1400), fastq_text(rng, 40)
    half = rng.integers(0, 256, size=20000, dtype=np.uint8).tobytes()
    noise = rng.integers(0, 256, size=200000, dtype=np.uint8).tobytes()
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    big_first = co.compress(b) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(noise) + co.flush()
    good = {"multi": (members([a, b, b"", a]), a + b + a), "bgzf": (bgzf_compress(a), a), "cross": (gz_level(a + half + half + b, 6), a + half + half + b),
            "grow": (big_first, b + noise)}
    gz = good["multi"][0]
    flipped = bytearray(gz); flipped[len(gz) // 2] ^= 0x10
    crc = bytearray(gz); crc[-8] ^= 1
    bad = {"flipped": bytes(flipped), "crc": bytes(crc), "truncated": gz[:-3], "garbage": gz + b"garbage", "half": gz[:len(gz) // 2]}
    args = []
    for name, (g, t) in good.items():
        (tmp_path / (name + ".gz")).write_bytes(g)
        (tmp_path / (name + ".txt")).write_bytes(t)
        args += ["good", str(tmp_path / (name + ".gz")), str(tmp_path / (name + ".txt"))]
    for name, g in bad.items():
        (tmp_path / (name + ".gz")).write_bytes(g)
        args += ["bad", str(tmp_path / (name + ".gz")), str(tmp_path / "multi.txt")]
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "inflate stream sanitize run ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
