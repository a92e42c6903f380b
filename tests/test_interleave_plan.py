"""CPU tests of the interleaved-pair bookkeeping (sylph_amd/csrc/interleave_plan.h, the very header the mate-check kernel and the
host's roads include, compiled with g++ through tests/interleave_plan_capi.cpp): the mate rule on its named cases, the record
arithmetic, a numpy restatement of the rule over a few thousand random header pairs — the sequential rule and the kernel's group
walk both — and the stand-alone sanitizer run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from .helpers import build_path

HERE = os.path.dirname(os.path.abspath(__file__))
HDR = os.path.join(HERE, "..", "sylph_amd", "csrc", "interleave_plan.h")
SRC = os.path.join(HERE, "interleave_plan_capi.cpp")
u64, u32, i32, vp = C.c_uint64, C.c_uint32, C.c_int, C.c_void_p


@pytest.fixture(scope="module")
def L():
    out, stale = build_path("sylph_interleave_plan", [SRC, HDR], ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, SRC])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    for name in ("ip_pairs_of", "ip_kept_record", "ip_mean_record"):
        getattr(lib, name).restype = u64
        getattr(lib, name).argtypes = [u64]
    lib.ip_mean_stride.restype = u64
    lib.ip_record_of.restype = u64
    lib.ip_record_of.argtypes = [u64, u32]
    lib.ip_group_lanes.restype = u32
    lib.ip_id_len.restype = u64
    lib.ip_id_len.argtypes = [C.c_char_p, u64]
    lib.ip_mates.restype = i32
    lib.ip_mates.argtypes = [C.c_char_p, u64, C.c_char_p, u64]
    lib.ip_header_mates.restype = i32
    lib.ip_header_mates.argtypes = [C.c_char_p, u64, C.c_char_p, u64]
    lib.ip_group_mates.restype = i32
    lib.ip_group_mates.argtypes = [C.c_char_p, u64, C.c_char_p, u64, vp]
    return lib


def id_of(header: bytes) -> bytes:
    """the rule restated: the header up to the first space, tab, '\\r' or line end"""
    a = np.frombuffer(header, dtype=np.uint8)
    ends = np.flatnonzero(np.isin(a, np.frombuffer(b" \t\r\n", dtype=np.uint8)))
    return header[:int(ends[0])] if len(ends) else header


def mates_np(ha: bytes, hb: bytes) -> bool:
    a, b = id_of(ha), id_of(hb)
    if a == b:
        return True
    return a.endswith(b"/1") and b.endswith(b"/2") and a[:-2] == b[:-2]


def both(L, ha: bytes, hb: bytes):
    steps = u32(0)
    seq = L.ip_header_mates(ha, len(ha), hb, len(hb))
    grp = L.ip_group_mates(ha, len(ha), hb, len(hb), C.addressof(steps))
    assert seq == grp, (ha, hb, seq, grp)
    return bool(seq), steps.value


NAMED = [
    (b"read7", b"read7", True),                      # equal ids
    (b"read7/1", b"read7/2", True),                  # /1 /2
    (b"read7/2", b"read7/1", False),                 # /2 /1
    (b"SRR1.1", b"SRR1.2", False),                   # .1 .2: two spots
    (b"x/1", b"y/2", False),
    (b"/1", b"/2", True),                            # alone: the prefix is empty
    (b"", b"", True),                                # empty ids are equal ids
    (b"", b"a", False),
    (b"a", b"", False),
    (b" one", b"\ttwo", True),                       # both ids empty
    (b"r 1:N:0:ACGT", b"r 2:N:0:ACGT", True),        # cut at a space (the Illumina style)
    (b"r\t1", b"r 2", True),                         # cut at a tab against a space
    (b"r/1 left", b"r/2\tright", True),
    (b"wholeheaderisid", b"wholeheaderisid", True),  # a header that is all id
    (b"1", b"2", False),                             # length 1
    (b"a", b"a", True),
    (b"a1", b"a2", False),                           # length 2, no slash
    (b"ab", b"ab", True),
    (b"r\r", b"r", True),                            # a '\r' is not part of an id
    (b"r/1\r\n", b"r/2\r\n", True),
    (b"r/1\r", b"r/2", True),
    (b"r/1x", b"r/2x", False),                       # not at the end
    (b"r/1", b"r/3", False),
    (b"r/1", b"r/22", False),
    (b"ra", b"r", False),
]


@pytest.mark.parametrize("ha,hb,want", NAMED)
def test_mates_named_cases(L, ha, hb, want):
    assert mates_np(ha, hb) == want                  # (the restatement agrees with what the issue names)
    assert both(L, ha, hb)[0] == want
    a, b = id_of(ha), id_of(hb)
    assert L.ip_id_len(ha, len(ha)) == len(a) and L.ip_id_len(hb, len(hb)) == len(b)
    assert bool(L.ip_mates(a, len(a), b, len(b))) == want


def test_id_len_lengths_0_1_2(L):
    assert L.ip_id_len(b"", 0) == 0
    for h, n in ((b"a", 1), (b" ", 0), (b"\t", 0), (b"\r", 0), (b"\n", 0), (b"ab", 2), (b"a ", 1), (b" a", 0), (b"a\t", 1), (b"a\r", 1)):
        assert L.ip_id_len(h, len(h)) == n
    assert L.ip_id_len(b"abc def", 2) == 2           # n bounds the walk


def test_pairs_and_kept_record(L):
    assert L.ip_mean_stride() == 2
    for n in list(range(6)) + [2**32 - 1, 2**32, 2**32 + 1, 2**64 - 2, 2**64 - 1]:
        assert L.ip_pairs_of(n) == n // 2
        assert L.ip_kept_record(n) == 2 * (n // 2)
        assert L.ip_kept_record(n) % 2 == 0 and n - L.ip_kept_record(n) in (0, 1)
    assert [L.ip_pairs_of(n) for n in range(6)] == [0, 0, 1, 1, 2, 2]
    assert [L.ip_kept_record(n) for n in range(6)] == [0, 0, 2, 2, 4, 4]
    for p in (0, 1, 2, 2**32, 2**62):
        assert L.ip_mean_record(p) == 2 * p == L.ip_record_of(p, 0) and L.ip_record_of(p, 1) == 2 * p + 1


def test_random_header_pairs_against_numpy(L):
    rng = np.random.default_rng(20)
    G = L.ip_group_lanes()
    alphabet = np.frombuffer(b"ACGT0129/._: \t\r", dtype=np.uint8)
    n_yes = n_multi = 0
    for i in range(4000):
        kind = i % 6
        la = int(rng.integers(0, 101)) if i % 5 else int(rng.choice([0, 1, 2, G - 1, G, G + 1, 2 * G, 2 * G + 1]))
        a = bytearray(rng.choice(alphabet[:12] if kind >= 2 else alphabet, size=la).tobytes())
        b = bytearray(a)
        if kind == 1 and la:
            b[int(rng.integers(0, la))] = ord("Z")
        elif kind == 2:
            at = int(rng.integers(0, la + 1))
            a[at:at] = b"/1"
            b[at:at] = b"/2"
        elif kind == 3:
            a += b"/1"
            b += b"/2"
        elif kind == 4:
            a += b"/1 left"
            b += b"/2\tright words"
        elif kind == 5:
            b += bytes(rng.choice(alphabet, size=1))
        got, steps = both(L, bytes(a), bytes(b))
        assert got == mates_np(bytes(a), bytes(b)), (bytes(a), bytes(b))
        n_yes += got
        n_multi += steps > 1
    assert 1000 < n_yes < 3500 and n_multi > 500         # both verdicts and more than one step are well covered


def test_group_walk_reads_nothing_behind_the_step_in_which_an_id_ends(L):
    G = L.ip_group_lanes()
    for n in (0, 1, G - 1, G, G + 1, 3 * G):
        h = b"q" * n + b" " + b"x" * 500
        got, steps = both(L, h, h)
        assert got and steps == n // G + 1
    got, steps = both(L, b"a" + b"q" * 300, b"b" + b"q" * 300)    # ids that differ in anything but a /1 against a /2: decided at once
    assert not got and steps == 1
    got, steps = both(L, b"r/1" + b"q" * 300, b"r/2" + b"q" * 300)   # a /1 against a /2 may be the ids' end: the walk goes on to the ends
    assert not got and steps == 303 // G + 1


def test_standalone_program_runs_clean_under_the_sanitizers():
    """tests/interleave_plan_sanitize_main.cpp + the model, built with AddressSanitizer and UBSan into a program of its own and run
    on the CPU: nothing is loaded into this interpreter."""
    srcs = [os.path.join(HERE, "interleave_plan_sanitize_main.cpp"), SRC]
    exe, stale = build_path("sylph_interleave_plan_sanitize", srcs + [HDR])
    if stale:
        tmp = exe + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                               "-Werror", "-o", tmp] + srcs)
        os.replace(tmp, exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "interleave plan sanitize run ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    assert " 0 cases" not in p.stdout and " 0 mates" not in p.stdout and " 0 of more" not in p.stdout
