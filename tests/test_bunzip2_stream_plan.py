"""The streamed bzip2 decoder's bookkeeping (sylph_amd/csrc/bunzip2_stream_plan.h, the very header csrc/bunzip2.hip includes) on the
CPU: the carry, the cut and the sliced chain walk, driven one slice per call by the CPU model of the kernels' reports
(tests/bunzip2_stream_plan_capi.cpp, which reuses bunzip2_plan_capi.cpp's).  The model reports where blocks end, not their bytes: every
chain block the walk hands out is decoded here by libbz2 as a one-block stream of its own (block_text), and the blocks put together must
equal bz2.decompress of the file.  The device side is tests/test_gpu_bunzip2_stream.py."""
import bz2
import ctypes as C
import os
import subprocess

import pytest

from .bunzip2_stream_inputs import block_text, eos_crc_bit, flip, magic_bits, packed, texts
from .helpers import build_path

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "sylph_amd", "csrc")
SRCS = [os.path.join(HERE, "bunzip2_stream_plan_capi.cpp")]
HEADERS = [os.path.join(HERE, "bunzip2_plan_capi.cpp")] + [os.path.join(CSRC, h) for h in ("bunzip2_stream_plan.h", "bunzip2_plan.h", "stream_plan.h")]
KiB = 1 << 10


@pytest.fixture(scope="module")
def plan():
    out, stale = build_path("sylph_bunzip2_stream_plan", SRCS + HEADERS, ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, SRCS[0]])
        os.replace(tmp, out)
    L = C.CDLL(out)
    u64p = C.POINTER(C.c_uint64)
    L.bsp_cut.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, u64p]
    L.bsp_cut.restype = None
    L.bsp_overlap.restype = C.c_uint64
    L.bsp_min_slice.restype = C.c_uint64
    L.bsp_open.restype = C.c_void_p
    L.bsp_open.argtypes = [C.POINTER(C.c_char_p), u64p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32]
    L.bsp_close.argtypes = [C.c_void_p]
    L.bsp_close.restype = None
    L.bsp_next.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), u64p, C.c_uint32, u64p, C.c_uint32, C.POINTER(C.c_uint32), u64p, C.POINTER(C.c_uint8), u64p,
                           C.c_char_p, C.c_size_t]
    return L


class Model:
    """the host half of a stream over the model; next() -> per file the text of the step's blocks (decoded by libbz2), or raises ValueError"""

    def __init__(self, plan, files, slice_bytes, overlap=0, batch=1000):
        self.L, self.files = plan, list(files)
        self.bufs = (C.c_char_p * len(files))(*files)
        self.sizes = (C.c_uint64 * len(files))(*[len(f) for f in files])
        self.h = plan.bsp_open(self.bufs, self.sizes, len(files), slice_bytes, overlap, batch)
        self.ints = [int.from_bytes(f, "big") for f in files]
        self.finished = [False] * len(files)
        self.state = [(0, 0, 0, 0, 0, 0)] * len(files)
        self.blocks = []                       # (file, start bit, end bit) of every chain block so far
        self.slices = self.peak_upload = self.decoded = 0

    def next(self, advance=None, extra=()):
        F, cap = len(self.files), 256
        adv = (C.c_uint8 * F)(*advance) if advance is not None else None
        ex = (C.c_uint64 * max(2, 2 * len(extra)))(*[v for pair in extra for v in pair])
        blk, n_blk = (C.c_uint64 * (4 * cap))(), C.c_uint32(0)
        state, fin, info = (C.c_uint64 * (6 * F))(), (C.c_uint8 * F)(), (C.c_uint64 * 3)()
        err = C.create_string_buffer(256)
        if self.L.bsp_next(self.h, adv, ex, len(extra), blk, cap, C.byref(n_blk), state, fin, info, err, 256) != 0:
            raise ValueError(err.value.decode())
        assert n_blk.value <= cap
        out = [b""] * F
        for k in range(n_blk.value):
            f, start, end, crc = (int(v) for v in blk[4 * k:4 * k + 4])
            self.blocks.append((f, start, end))
            out[f] += block_text(self.ints[f], len(self.files[f]) * 8, start, end)
        self.finished = [bool(v) for v in fin]
        self.state = [tuple(int(v) for v in state[6 * f:6 * f + 6]) for f in range(F)]
        self.slices, self.peak_upload, self.decoded = int(info[0]), int(info[1]), int(info[2])
        return out

    def close(self):
        self.L.bsp_close(self.h)


def run(plan, files, slice_bytes, order="together", **kw):
    """all windows of every file put together; order: the files advance together, or alternately"""
    m = Model(plan, files, slice_bytes, **kw)
    got = [b""] * len(files)
    try:
        turn = 0
        while not all(m.finished):
            adv = None
            if order == "alternately" and len(files) > 1:
                live = [f for f in range(len(files)) if not m.finished[f]]
                adv = [int(f == live[turn % len(live)]) for f in range(len(files))]
            for f, t in enumerate(m.next(adv)):
                got[f] += t
            turn += 1
            assert turn < 10000
        return got, m
    finally:
        m.close()


def test_the_cut_rule(plan):
    MiB = 1 << 20
    assert plan.bsp_overlap() == MiB and plan.bsp_min_slice() == 64 * KiB
    assert MiB >= 909_600                          # libbz2's largest block: 1.01 x 900 000 + 600 bytes

    def cut(bit, n, s):
        o = (C.c_uint64 * 3)()
        plan.bsp_cut(bit, n, s, o)
        return tuple(int(v) for v in o)
    assert cut(0, 10 * MiB, 2 * MiB) == (0, 2 * MiB, 3 * MiB)
    assert cut(8 * 12345 + 3, 10 * MiB, 2 * MiB) == (12345, 12345 + 2 * MiB, 12345 + 3 * MiB)       # pos: the byte of the carry's bit
    assert cut(0, 10 * MiB, 1) == (0, 64 * KiB, 64 * KiB + MiB)                                   # a slice is at least 64 KiB
    assert cut(0, 100, 64 * KiB) == (0, 100, 100)                                                 # the file ends in the slice
    assert cut(8 * 9 * MiB, 10 * MiB, 512 * KiB) == (9 * MiB, 9 * MiB + 512 * KiB, 10 * MiB)      # ... in the overlap
    assert cut(8 * 10 * MiB, 10 * MiB, 512 * KiB) == (10 * MiB, 10 * MiB, 10 * MiB)


@pytest.mark.parametrize("level", [1, 9])
@pytest.mark.parametrize("slice_kib", [64, 128, 256])
def test_windows_put_together_equal_libbz2(plan, level, slice_kib):
    t = texts()
    for name in ("fastq", "noise", "runs"):
        data = packed(name, level)
        (got,), m = run(plan, [data], slice_kib * KiB)
        assert got == t[name] == bz2.decompress(data), name
        assert m.state[0][4] == 1 and m.state[0][5] == len(magic_bits(data)), name
        assert m.slices >= (len(data) // (slice_kib * KiB) if (name, level) == ("fastq", 1) else 1), name
        assert m.peak_upload <= slice_kib * KiB + plan.bsp_overlap()
    # a block larger than the slice lives in the overlap: noise at -1 is blocks of ~100 kB
    if level == 1 and slice_kib == 64:
        bits = magic_bits(packed("noise", 1))
        assert len(bits) >= 3 and bits[1] // 8 - bits[0] // 8 > 64 * KiB
    # two files, advancing together and alternately
    files = [packed("fastq", level), packed("fastq2", level)]
    for order in ("together", "alternately"):
        got, _ = run(plan, files, slice_kib * KiB, order)
        assert got[0] == t["fastq"] and got[1] == t["fastq2"], order


def test_small_batches_of_reports(plan):
    data = packed("fastq", 1)
    for batch in (1, 3):
        (got,), _ = run(plan, [data], 128 * KiB, batch=batch)
        assert got == texts()["fastq"]


def test_stream_boundary_at_and_beside_a_slice_end(plan):
    """the first stream ends 0, -1 and +1 bytes from the first slice's nominal cut; the cut falls on the next stream's header, inside
    it, and in front of the end-of-stream trailer"""
    t = texts()
    a = packed("fastq", 1)
    b = bz2.compress(t["fastq2"], 1)
    for slice_bytes in (len(a), len(a) + 1, len(a) - 1, len(a) + 2, len(a) - 10, len(a) - 11):
        assert slice_bytes >= 64 * KiB
        (got,), m = run(plan, [a + b], slice_bytes)
        assert got == t["fastq"] + t["fastq2"], slice_bytes - len(a)
        assert m.state[0][4] == 2


def test_empty_stream_between_two_others_and_many_streams(plan):
    t = texts()
    data = packed("fastq", 1) + bz2.compress(b"", 9) + packed("fastq2", 9) + bz2.compress(b"", 1) + bz2.compress(b"", 1) + packed("noise", 1)
    for slice_kib in (64, 256):
        (got,), m = run(plan, [data], slice_kib * KiB)
        assert got == t["fastq"] + t["fastq2"] + t["noise"] == bz2.decompress(data)
        assert m.state[0][4] == 6
    (got,), m = run(plan, [bz2.compress(b"", 9)], 64 * KiB)
    assert got == b"" and m.state[0][4:6] == (1, 0)


def test_a_stream_over_three_slices_has_its_combined_crc_checked_where_it_ends(plan):
    data = packed("fastq", 1)
    assert len(data) > 3 * 64 * KiB
    m = Model(plan, [data], 64 * KiB)
    try:
        combined = []
        while not m.finished[0]:
            m.next()
            combined.append((m.state[0][1], m.state[0][3]))
        assert m.slices >= 3 and all(in_stream for in_stream, _ in combined[:-1]) and len({c for _, c in combined[:-1]}) == len(combined) - 1
    finally:
        m.close()
    # one flipped bit in the stream's combined CRC: every slice but the last walks, the last one declines
    bad = flip(data, eos_crc_bit(data) + 9)
    m = Model(plan, [bad], 64 * KiB)
    try:
        got = b""
        with pytest.raises(ValueError, match="combined CRC"):
            while not m.finished[0]:
                got += m.next()[0]
        assert m.slices >= 3 and texts()["fastq"].startswith(got) and len(got) > len(texts()["fastq"]) // 2
    finally:
        m.close()


def test_injected_false_candidates(plan):
    data = packed("fastq", 1)
    bits = magic_bits(data)
    m = Model(plan, [data], 64 * KiB, batch=2)
    try:
        got = b""
        while not m.finished[0]:
            at = m.state[0][0]
            # on the chain (a true block's own bit, twice), off it, and at the first bits of the slice (in front of the carry's bit too)
            extra = [(0, bits[3]), (0, bits[3]), (0, bits[5] + 1), (0, at // 8 * 8), (0, at + 1), (0, at + 4000), (0, at + 64 * KiB * 8 + 99)]
            got += m.next(None, extra)[0]
        assert got == texts()["fastq"]
        assert [b[1] for b in m.blocks] == bits
    finally:
        m.close()


def test_overrun_at_a_slice_end_is_the_cut_at_the_files_end_damage_past_the_overlap_declined(plan):
    t = texts()
    # an overlap of 50 kB: noise's second block (-1: ~100 kB each) starts behind the first slice's cut, inside the uploaded bytes, and
    # runs out of them — the decoder's overrun there is the cut, and the next slice begins with that block
    data = packed("noise", 1)
    (got,), m = run(plan, [data], 64 * KiB, overlap=50_000)
    assert got == t["noise"] and m.slices >= 3
    # the same report where the FILE ends is damage
    with pytest.raises(ValueError, match="status 21|past the end"):
        run(plan, [data[:-2000]], 64 * KiB)
    with pytest.raises(ValueError, match="status 21|past the end"):
        run(plan, [packed("fastq", 1)[:-200]], 64 * KiB)
    # a block that starts in front of the cut and overruns the overlap is declined: -9 noise is one block of ~300 kB
    one = packed("noise", 9)
    assert len(magic_bits(one)) == 1
    with pytest.raises(ValueError, match="runs past its overlap"):
        run(plan, [one], 64 * KiB, overlap=100_000)
    (got,), _ = run(plan, [one], 64 * KiB)          # (the real overlap holds it)
    assert got == t["noise"]


def test_trailing_garbage_and_other_damage(plan):
    t = texts()
    good = packed("fastq", 1)
    bits = magic_bits(good)
    cases = {"trailing": (good + b"garbage!", "no bzip2 stream header"), "trailing_after_two": (good + packed("noise", 1) + b"\x00", "no bzip2 stream header"),
             "truncated": (good[:len(good) * 2 // 3], "status|past the end|is no candidate|chain breaks"),
             "randomised": (flip(good, bits[8] + 80), "randomised"), "late_magic": (flip(good, bits[10] + 3), "chain breaks")}
    for name, (data, why) in cases.items():
        m = Model(plan, [data], 64 * KiB)
        try:
            got = b""
            with pytest.raises(ValueError, match=why):
                while not m.finished[0]:
                    got += m.next()[0]
            assert t["fastq"].startswith(got[:len(t["fastq"])]), name
            if name in ("randomised", "late_magic"):
                assert m.slices >= 2 and got, name       # the slices in front of the damage were handed out
        finally:
            m.close()
    with pytest.raises(ValueError, match="no bzip2 stream header"):
        run(plan, [b""], 64 * KiB)
    with pytest.raises(ValueError, match="no bzip2 stream header"):
        run(plan, [b"BZh0" + good[4:]], 64 * KiB)


def test_standalone_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/bunzip2_stream_sanitize_main.cpp + the model, built with AddressSanitizer and UBSan into a program of its own and run as a
    child process over inputs of the tests above: host code only, nothing is loaded into this interpreter."""
    main = os.path.join(HERE, "bunzip2_stream_sanitize_main.cpp")
    exe, stale = build_path("sylph_bunzip2_stream_sanitize", [main] + SRCS + HEADERS)
    if stale:
        tmp = exe + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                               "-o", tmp, main, SRCS[0]])
        os.replace(tmp, exe)
    good = packed("fastq", 1)
    multi = good + bz2.compress(b"", 9) + packed("noise", 1)
    inputs = [("good", good, 1, len(magic_bits(good))), ("good", multi, 3, len(magic_bits(multi))), ("good", packed("noise", 9), 1, 1),
              ("bad", good[:-100], 0, 0), ("bad", good + b"x", 0, 0), ("bad", flip(good, eos_crc_bit(good) + 3), 0, 0)]
    args = []
    for i, (kind, data, streams, blocks) in enumerate(inputs):
        p = tmp_path / f"{i}.bz2"
        p.write_bytes(data)
        args += [kind, str(p), str(streams), str(blocks)]
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "bunzip2 stream sanitize run ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
