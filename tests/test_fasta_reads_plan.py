"""CPU tests of the bookkeeping of FASTA-format reads (sylph_amd/csrc/fasta_reads_plan.h, the very header fa_batch_kernel of
csrc/fasta.hip includes, compiled with g++ through tests/fasta_reads_plan_capi.cpp into a sequential model of that kernel): every output
byte of a batch must come from the (mate, record, offset) a Python model names, the gathered bytes must be the records side by side, the
window rule of sylph_fasta_index_window must hold at every cut of a text and windows fed one after the other must give the whole
text's records — and the model's stand-alone sanitizer run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from .fasta_texts import fasta_text
from .helpers import build_path

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "sylph_amd", "csrc")
HDRS = [os.path.join(CSRC, "fasta_reads_plan.h"), os.path.join(CSRC, "fasta_plan.h")]
CAPI = os.path.join(HERE, "fasta_reads_plan_capi.cpp")
ERR_FORMAT = -5
LENGTHS = [0, 1, 15, 16, 17, 4095, 4096, 4097, 20000]


@pytest.fixture(scope="module")
def L():
    out, stale = build_path("sylph_fasta_reads_plan", [CAPI] + HDRS, ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, CAPI])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    vp, u64, u64p = C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)
    lib.fr_tile_bytes.restype = C.c_uint32
    lib.fr_batch_total.argtypes = [vp, vp, u64, u64]
    lib.fr_batch_total.restype = u64
    lib.fr_batch_map.argtypes = [vp, vp, u64, u64, vp, vp, vp, C.POINTER(C.c_uint32)]
    lib.fr_batch_map.restype = u64
    lib.fr_batch_gather.argtypes = [vp, u64, vp, vp, u64, vp, u64, u64, vp, u64]
    lib.fr_window.argtypes = [vp, u64, C.c_int, u64p, u64p]
    return lib


def make_file(rng, lens):
    """(joined bases, record offsets) of a file whose records have these lengths"""
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    return rng.choice(np.frombuffer(b"ACGTNacgt", dtype=np.uint8), size=int(off[-1])).astype(np.uint8), off


def model_batch(files, first, n_items):
    """[(mate, record, index in that file's joined bases)] for every byte of the batch, and the bytes themselves"""
    where, data = [], []
    for i in range(first, first + n_items):
        for m, (bases, off) in enumerate(files):
            a, b = int(off[i]), int(off[i + 1])
            where += [(m, i, x) for x in range(a, b)]
            data.append(bases[a:b])
    return where, np.concatenate(data + [np.zeros(0, np.uint8)])


def check_batch(L, files, first, n_items):
    where, want = model_batch(files, first, n_items)
    total = len(where)
    ro = [f[1] for f in files]
    pa, pb = ro[0].ctypes.data, (ro[1].ctypes.data if len(files) == 2 else None)
    assert L.fr_batch_total(pa, pb, first, n_items) == total
    mate, rec, src = np.full(total + 1, 9, np.uint8), np.zeros(total + 1, np.uint64), np.zeros(total + 1, np.uint64)
    pieces = C.c_uint32(0)
    assert L.fr_batch_map(pa, pb, first, n_items, mate.ctypes.data, rec.ctypes.data, src.ctypes.data, C.byref(pieces)) == 0, "a byte no lane, or two lanes, wrote"
    assert pieces.value <= 16
    got = list(zip(mate[:total].tolist(), rec[:total].tolist(), src[:total].tolist()))
    assert got == where
    cap = (total + 15) // 16 * 16
    mem = np.full(cap + 32, 0xEE, dtype=np.uint8)
    out = mem[(-mem.ctypes.data) % 16:]
    ja, jb = files[0][0], (files[1][0] if len(files) == 2 else np.zeros(0, np.uint8))
    assert L.fr_batch_gather(ja.ctypes.data, len(ja), pa, jb.ctypes.data if len(files) == 2 else None, len(jb), pb, first, n_items, out.ctypes.data, cap) == 0
    assert np.array_equal(out[:total], want)
    assert np.all(out[total:cap] == 0) and np.all(out[cap:cap + 16] == 0xEE), "only zeros up to the next 16-byte boundary, nothing behind it"
    return pieces.value


def the_lengths(rng, variant):
    """the issue's record lengths with runs of 40 one-base records and rows of empty ones between them"""
    lens = [1] * 40
    for n in LENGTHS:
        lens += [n + (variant if n > 1 else 0)] + [0] * int(rng.integers(0, 4))
    lens += [1] * 40 + [int(x) for x in rng.integers(0, 200, size=30)] + [0] * 20 + [1] * 17 + [5 + variant]
    return lens


@pytest.mark.parametrize("paired", [False, True])
def test_every_output_byte_comes_from_the_right_place(L, paired):
    assert L.fr_tile_bytes() == 4096
    rng = np.random.default_rng(5 + paired)
    files = [make_file(rng, the_lengths(rng, v)) for v in range(2 if paired else 1)]
    if paired:                                                              # (the two files hold the same number of records here)
        n = min(len(f[1]) for f in files) - 1
        files = [(b, o[:n + 1]) for b, o in files]
    n = len(files[0][1]) - 1
    most = 0
    for first, n_items in ((0, n), (0, 0), (n, 0), (0, 1), (3, 37), (39, 12), (41, n - 41), (n - 1, 1), (n // 2, n - n // 2)):
        most = max(most, check_batch(L, files, first, n_items))
    if not paired:
        assert most == 16, "a lane inside the run of one-base records crosses every boundary of its 16 bytes"


def test_record_lengths_around_the_lane_and_the_tile(L):
    """every one of the lengths alone, as the first and as the last record of a batch, whose last tile is partial unless the length says otherwise"""
    rng = np.random.default_rng(7)
    for n in LENGTHS:
        for lens in ([n], [n, 3], [3, n], [0, n, 0], [n, n]):
            f = make_file(rng, lens)
            check_batch(L, [f], 0, len(lens))
            check_batch(L, [f, make_file(rng, lens[::-1])], 0, len(lens))
            if len(lens) > 1:
                check_batch(L, [f], 1, len(lens) - 1)


def test_random_batches(L):
    rng = np.random.default_rng(8)
    for case in range(30):
        n = int(rng.integers(1, 300))
        mk = lambda: make_file(rng, [int(x) for x in rng.integers(0, int(rng.choice([3, 40, 700])), size=n)])
        files = [mk(), mk()] if case & 1 else [mk()]
        first = int(rng.integers(0, n + 1))
        check_batch(L, files, first, int(rng.integers(0, n - first + 1)))


# ---------------------------------------------------------------------------------------------------------------- the window rule
TEXT = fasta_text([b"ACGTACGTAC", b"", b"GGCCGGCCGGCCGGCCGGCCGGCCGG", b"A", b"", b"TTGACCA" * 9, b"ACGT"],
                  [b"r1 first", b"r2", b"r3 > @", b"", b"r5", b"r6", b"last"], width=11, eol=b"\r\n", blank_every=4) + \
    fasta_text([b"CCCCCCCCCCCCCCCCCCCCCCCCCCCCCC", b"G" * 45], [b"lf", b"lf2"], width=20, last_eol=False) + b"\r"


def python_records(text):
    """the records of a whole FASTA text: [(where its '>' lies, sequence)]"""
    recs = []
    pos = 0
    for line in text.split(b"\n"):
        if line.startswith(b">"):
            recs.append([pos, b""])
        elif recs:
            recs[-1][1] += line.rstrip(b"\r")
        pos += len(line) + 1
    return [(p, s) for p, s in recs]


def python_window(text, final):
    """(rc, records, consumed) by the issue's rule"""
    if not text:
        return (ERR_FORMAT, 0, 0) if final else (0, 0, 0)
    if text[:1] != b">" or any(text[i:i + 1] == b"\r" and text[i + 1:i + 2] != b"\n" for i in range(len(text) - 1)):
        return ERR_FORMAT, 0, 0
    heads = [p for p, _ in python_records(text)]
    if final:
        return 0, len(heads), len(text)
    return 0, max(0, len(heads) - 1), heads[-1] if len(heads) >= 2 else 0


def c_window(L, text, final):
    buf = np.frombuffer(text, dtype=np.uint8).copy() if text else np.zeros(1, np.uint8)
    r, u = C.c_uint64(0), C.c_uint64(0)
    rc = L.fr_window(buf.ctypes.data, len(text), final, C.byref(r), C.byref(u))
    return rc, r.value, u.value


def test_the_window_rule_at_every_cut(L):
    assert 250 <= len(TEXT) <= 400 and len(python_records(TEXT)) == 9
    for cut in range(len(TEXT) + 1):
        for final in (0, 1):
            assert c_window(L, TEXT[:cut], final) == python_window(TEXT[:cut], final), (cut, final)
    for bad in (b"ACGT\n>a\n", b"\n>a\nAC\n", b">a\nAC\rGT\n>b\n", b">a\r\r\n>b\n"):
        for final in (0, 1):
            assert c_window(L, bad, final)[0] == ERR_FORMAT == python_window(bad, final)[0]


@pytest.mark.parametrize("step", [1, 7, 64, 150, 1000])
def test_windows_fed_one_after_the_other_give_the_whole_texts_records(L, step):
    want = [s for _, s in python_records(TEXT)]
    got, tail, pos = [], b"", 0
    while True:
        tail += TEXT[pos:pos + step]
        pos += step
        final = int(pos >= len(TEXT))
        rc, n, used = c_window(L, tail, final)
        assert rc == 0
        recs = python_records(tail[:used])
        assert len(recs) == n
        got += [s for _, s in recs]
        tail = tail[used:]
        if final:
            break
    assert got == want


# ------------------------------------------------------------------------------------------------------------------- sanitizers
def test_standalone_program_runs_clean_under_the_sanitizers():
    """tests/fasta_reads_sanitize_main.cpp + the model, built with AddressSanitizer and UBSan into a program of its own and run on the
    CPU: nothing of it is loaded into this interpreter."""
    srcs = [os.path.join(HERE, "fasta_reads_sanitize_main.cpp"), CAPI]
    exe, stale = build_path("sylph_fasta_reads_sanitize", srcs + HDRS)
    if stale:
        tmp = exe + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                               "-Werror", "-o", tmp] + srcs)
        os.replace(tmp, exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "fasta reads sanitize run ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
