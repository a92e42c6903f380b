"""CPU tests of the FASTA index and join's bookkeeping (sylph_amd/csrc/fasta_plan.h, the very header the kernels of csrc/fasta.hip
include, compiled with g++ through tests/fasta_plan_capi.cpp into a sequential model of those kernels): the records the model finds and
the sequences it joins must be the ones oracle.read_fastx reads from the same bytes — over line widths, line ends, blank lines, empty
records and every alignment of the text and of its destination — and everything sylph_fasta_index refuses must be refused by the model."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from .fasta_texts import REFUSED, fasta_text, random_records, records_by_the_host_reader

HERE = os.path.dirname(os.path.abspath(__file__))
ERR_FORMAT = -5


@pytest.fixture(scope="module")
def L():
    out = os.path.join(tempfile.gettempdir(), f"sylph_fasta_plan_{os.getuid()}.so")
    src = os.path.join(HERE, "fasta_plan_capi.cpp")
    hdr = os.path.join(HERE, "..", "sylph_amd", "csrc", "fasta_plan.h")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, src])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    vp, u64, u64p = C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)
    lib.fa_max_text_bytes.restype = u64
    lib.fa_size_refused.argtypes = [u64, u64]
    lib.fa_index.argtypes = [vp, u64, C.c_uint32, C.POINTER(vp)]
    lib.fa_counts.argtypes = [vp, u64p, u64p, u64p, u64p]
    lib.fa_records.argtypes = [vp, vp, vp, vp]
    lib.fa_join.argtypes = [vp, vp, u64, u64, u64p, u64p, u64p]
    lib.fa_join.restype = C.c_uint32
    lib.fa_free.argtypes = [vp]
    lib.fa_free.restype = None
    return lib


def model_records(L, text, bias=0, out_pos=0):
    """(rc, [(id, sequence)], stats) as the model of the kernels finds and joins them"""
    buf = np.frombuffer(text, dtype=np.uint8).copy() if len(text) else np.zeros(1, dtype=np.uint8)
    h = C.c_void_p()
    rc = L.fa_index(buf.ctypes.data, len(text), bias, C.byref(h))
    if rc != 0:
        assert not h
        return rc, None, None
    nr, nb, ni, nl = (C.c_uint64(0) for _ in range(4))
    L.fa_counts(h, C.byref(nr), C.byref(nb), C.byref(ni), C.byref(nl))
    nr, nb, ni = nr.value, nb.value, ni.value
    rec_off, id_pos, id_len = np.zeros(nr + 1, np.uint64), np.zeros(max(1, nr), np.uint64), np.zeros(max(1, nr), np.uint32)
    L.fa_records(h, rec_off.ctypes.data, id_pos.ctypes.data, id_len.ctypes.data)
    # (the model takes its memory as 16-byte aligned: numpy's allocation need not be, so hand it an aligned window; 64 guard bytes)
    mem = np.full(out_pos + nb + 64 + 32, 0xEE, dtype=np.uint8)
    win = mem[(-mem.ctypes.data) % 16:]
    wide, narrow, outside = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    err = L.fa_join(h, win.ctypes.data, len(win), out_pos, C.byref(wide), C.byref(narrow), C.byref(outside))
    L.fa_free(h)
    assert err == 0 and outside.value == 0
    assert np.all(win[:out_pos] == 0xEE) and np.all(win[out_pos + nb:] == 0xEE), "the join wrote outside its bases"
    assert int(rec_off[0]) == 0 and int(rec_off[nr]) == nb and int(id_len[:nr].sum()) == ni
    joined = win[out_pos:out_pos + nb].tobytes()
    recs = [(text[int(id_pos[r]):int(id_pos[r]) + int(id_len[r])], joined[int(rec_off[r]):int(rec_off[r + 1])]) for r in range(nr)]
    return 0, recs, dict(wide=wide.value, narrow=narrow.value, n_bases=nb, n_lines=nl.value)


SHAPES = [(w, eol, last_eol, trailing, blank)
          for w in (1, 2, 15, 16, 17, 60, 80, 200, 0)
          for eol, last_eol, trailing, blank in ((b"\n", True, 0, 0), (b"\n", False, 0, 0), (b"\r\n", True, 0, 3), (b"\r\n", False, 0, 0),
                                                 (b"\n", True, 3, 7), (b"\r\n", True, 2, 0))]


@pytest.mark.parametrize("width,eol,last_eol,trailing,blank", SHAPES)
def test_model_finds_the_host_readers_records(L, tmp_path, width, eol, last_eol, trailing, blank):
    rng = np.random.default_rng(1000 + width * 7 + len(eol) + 2 * last_eol + trailing + blank)
    recs, ids = random_records(rng, 60, max_len=300 if width != 1 else 120)
    recs[0], recs[30], recs[-1] = b"", b"", b""                                # an empty record first, in the middle and last
    recs[7] = b"A"
    text = fasta_text(recs, ids, width=width, eol=eol, last_eol=last_eol, trailing=trailing, blank_every=blank)
    want = records_by_the_host_reader(text, tmp_path)
    assert [s for _, s in want] == recs and [i for i, _ in want] == ids      # (the generator and the reader agree on what was written)
    for bias, out_pos in ((0, 0), (1, 1), (15, 15), (7, 4097)):
        rc, got, _ = model_records(L, text, bias, out_pos)
        assert rc == 0
        assert got == want, (bias, out_pos)


def test_random_line_widths_and_every_alignment(L, tmp_path):
    """line widths drawn from 1..200 per text, every bias of the text against the 16-byte stream and every alignment of the destination"""
    rng = np.random.default_rng(7)
    for case in range(16):
        recs, ids = random_records(rng, int(rng.integers(1, 40)), max_len=int(rng.integers(1, 3000)))
        text = fasta_text(recs, ids, width=int(rng.integers(1, 201)), eol=(b"\n", b"\r\n")[case & 1], last_eol=bool(case & 2),
                          trailing=int(rng.integers(0, 3)) if case & 4 else 0, blank_every=int(rng.integers(0, 5)))
        want = records_by_the_host_reader(text, tmp_path)
        assert [s for _, s in want] == recs
        rc, got, _ = model_records(L, text, case, 15 - case)
        assert rc == 0 and got == want, case


def test_long_single_line_records_and_tiles_of_newlines(L, tmp_path):
    """a 70,000-base record on one line spans 17 tiles; a record of 1-byte lines makes tiles of nearly all newlines; the stores are wide"""
    rng = np.random.default_rng(8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    long_rec = bytes(rng.choice(acgt, size=70000).astype(np.uint8))
    short = bytes(rng.choice(acgt, size=9000).astype(np.uint8))
    for eol in (b"\n", b"\r\n"):
        text = fasta_text([long_rec], [b"chr1"], width=0, eol=eol) + fasta_text([short], [b"one per line"], width=1, eol=eol) + \
            fasta_text([long_rec[:5000]], [b"tail"], width=60, eol=eol, last_eol=False)
        want = records_by_the_host_reader(text, tmp_path)
        assert [s for _, s in want] == [long_rec, short, long_rec[:5000]]
        rc, got, st = model_records(L, text, 3, 5)
        assert rc == 0 and got == want
        n_tiles = (len(text) + 3 + 4095) // 4096
        assert st["narrow"] <= 30 * n_tiles and st["wide"] * 16 + st["narrow"] == st["n_bases"]


def test_a_cr_at_the_very_end_belongs_to_the_line_end(L, tmp_path):
    for text in (b">a\nACGT\r", b">a\r\nAC\r\nGT\r", b">a\r", b">a b\r\n\r\n\r\n", b">"):
        want = records_by_the_host_reader(text, tmp_path)
        for bias in range(16):
            rc, got, _ = model_records(L, text, bias, bias)
            assert rc == 0 and got == want, (text, bias)


def test_line_ends_on_every_lane_and_tile_boundary(L, tmp_path):
    """CR LF pairs, headers and line starts moved across the 16-byte lane and the 4 KiB tile boundaries byte by byte"""
    seq = b"ACGTTGCA" * 40
    for pad in range(0, 34):
        head = b">" + b"x" * (4096 - 40 + pad)
        text = head + b"\r\n" + seq[:pad] + b"\r\n" + b">\r\n" + seq + b"\r\n\r\n>last @ >\r\n" + seq[:17]
        want = records_by_the_host_reader(text, tmp_path)
        rc, got, _ = model_records(L, text, pad % 16, (3 * pad) % 16)
        assert rc == 0 and got == want, pad


def test_what_the_index_refuses_the_model_refuses(L):
    for name, text in REFUSED.items():
        for bias in (0, 5, 15):
            rc, got, _ = model_records(L, text, bias)
            assert rc == ERR_FORMAT and got is None, name
    # a stray '\r' as the last byte of a lane and of a tile, with text behind it
    for at in (15, 16, 4095, 4096, 4097):
        text = b">a\n" + b"A" * (at - 3) + b"\r" + b"C" * 50 + b"\n"
        assert model_records(L, text)[0] == ERR_FORMAT, at
        ok = text[:at] + b"\n" + text[at + 1:]
        assert model_records(L, ok)[0] == 0, at
    # sizes: 2^32 - 4096 bytes or more, 2^32 lines or more (nothing of such a text is read)
    cap = L.fa_max_text_bytes()
    assert cap == 2**32 - 4096
    assert L.fa_size_refused(cap, 0) and L.fa_size_refused(2**40, 0) and L.fa_size_refused(0, 0)
    assert not L.fa_size_refused(cap - 1, 0)
    assert L.fa_size_refused(1000, 2**32 - 1) and not L.fa_size_refused(1000, 2**32 - 2)
    tiny = np.frombuffer(b">a\nACGT\n", dtype=np.uint8).copy()
    h = C.c_void_p()
    assert L.fa_index(tiny.ctypes.data, cap, 0, C.byref(h)) == ERR_FORMAT and not h
