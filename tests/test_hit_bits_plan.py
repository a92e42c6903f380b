"""CPU tests of the read kernel's hit bits as LDS atomics leave them (sylph_amd/csrc/seed_plan.h "hit bits set by LDS atomics", compiled
with g++ through tests/hit_bits_capi.cpp): every k-mer below the threshold xors hit_const(T) — its bit in BOTH halves of the group's word
— into a zeroed column, the lower half is cleared behind every even group, and count_hits decodes each word once.  For every number of
half-groups a wavefront can walk (0..48) and all-ones, all-zeros, single-bit and random hit patterns, the decoded column must be the
kmer_word / kmer_bit image bit for bit, for the wavefront's longest record and for shorter ones beside it, and tail_mask must clear from
the last word what it always cleared.

hit_decode is its own inverse: a second decode is NOT harmless (it returns the encoded word, shown below on every word with an odd
group's hit), which is why count_hits decodes under a flag that only the first round of a pass sets."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

from . import seed_plan_lib as SP

HERE = os.path.dirname(os.path.abspath(__file__))
MASKW = 12


@pytest.fixture(scope="module")
def H():
    src = os.path.join(HERE, "hit_bits_capi.cpp")
    hdr = os.path.join(HERE, "..", "sylph_amd", "csrc", "seed_plan.h")
    key = hashlib.sha256(open(src, "rb").read() + open(hdr, "rb").read()).hexdigest()[:16]
    out = os.path.join(tempfile.gettempdir(), f"sylph_hit_bits_{os.getuid()}_{key}.so")
    if not os.path.exists(out):
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, src])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    u8p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    for name, n in (("hb_const", 1), ("hb_decode", 1), ("hb_cleared", 1), ("hb_word_offset", 2), ("hb_group_half", 2)):
        getattr(lib, name).restype = C.c_uint32
        getattr(lib, name).argtypes = [C.c_uint32] * n
    lib.hb_clear_after.argtypes = [C.c_uint32]
    lib.hb_encode.argtypes = [u8p, C.c_uint32, u32p]
    lib.hb_encode.restype = None
    lib.hb_count.argtypes = [u32p, C.c_uint32, C.c_uint32]
    lib.hb_count.restype = C.c_uint32
    return lib


@pytest.fixture(scope="module")
def L():
    assert SP.constants()["MASKW"] == MASKW
    return SP.load()


def image(L, hits, nh):
    """the column count_hits must leave for a record of nh k-mers: kmer_word / kmer_bit, nothing at or beyond nh"""
    words = [0] * L.sp_mask_words(nh)
    for i in np.flatnonzero(hits[:nh]).tolist():
        words[L.sp_kmer_word(i)] |= 1 << L.sp_kmer_bit(i)
    return words


def encode(H, hits, n_half):
    col = (C.c_uint32 * (MASKW + 1))(*([0xDEADBEEF] * (MASKW + 1)))            # whatever the last pass left: the model zeroes its rows
    buf = np.ascontiguousarray(np.concatenate([hits, np.zeros(16, np.uint8)]))   # (a lone half-group reads 8 of a group's 16)
    H.hb_encode(buf.ctypes.data_as(C.POINTER(C.c_uint8)), n_half, col)
    return col


def check(H, L, hits, n_half, nh_list):
    enc = list(encode(H, hits, n_half))
    rows = L.sp_rows_used(n_half)
    assert enc[rows:] == [0xDEADBEEF] * (MASKW + 1 - rows), n_half               # nothing written above the pass's rows
    for nh in nh_list:
        col = (C.c_uint32 * (MASKW + 1))(*enc)
        cnt = H.hb_count(col, nh, 1)
        want = image(L, hits, nh)
        assert list(col)[:len(want)] == want, (n_half, nh)
        assert cnt == int(hits[:nh].sum()), (n_half, nh)
        assert list(col)[len(want):] == enc[len(want):], (n_half, nh)            # the words above the record's own are not touched


def nh_choices(n_half, rng):
    """k-mers of a record in a wavefront that walks n_half half-groups: the longest there can be, the lengths that end in every place of
    the last half-group, shorter neighbours, none"""
    top = min(8 * n_half, 380)
    out = {top, 0, *range(max(top - 8, 0), top + 1)}
    out |= {int(x) for x in rng.integers(0, top + 1, size=6)}
    return sorted(out)


def test_the_constants_and_the_word_of_a_group(H, L):
    for t in range(16):
        v = H.hb_const(t)
        assert v == ((1 << (15 - t)) | (1 << (31 - t))), t
        # the upper copy is the bit of k-mer t of an even group, the lower copy the bit of k-mer t of the odd group behind it
        assert v >> 16 << 16 == 1 << L.sp_kmer_bit(t) and v & 0xFFFF == 1 << L.sp_kmer_bit(16 + t), t
    for tpb in (256, 512):
        for g in range(24):
            assert H.hb_word_offset(g, tpb) == L.sp_kmer_word(16 * g) * tpb * 4, (g, tpb)
            # group_half counts 16-bit halves from the same base: the word's lower half at its offset, the upper two bytes on
            assert H.hb_group_half(g, tpb) * 2 == H.hb_word_offset(g, tpb) + (2 if g % 2 == 0 else 0), (g, tpb)
            assert H.hb_clear_after(g) == (g % 2 == 0)
    assert H.hb_cleared(0xFFFFFFFF) == 0xFFFF0000 and H.hb_cleared(0x1234ABCD) == 0x12340000


@pytest.mark.parametrize("n_half", range(0, 49))
def test_encode_clear_decode_is_the_mask_layout(H, L, n_half):
    rng = np.random.default_rng(1400 + n_half)
    n = 8 * n_half
    nhs = nh_choices(n_half, rng)
    check(H, L, np.ones(n, np.uint8), n_half, nhs)                   # both halves of every word full: the decode's worst case
    check(H, L, np.zeros(n, np.uint8), n_half, nhs)
    for p in (0.5, 0.05, 0.005):
        for _ in range(3):
            check(H, L, (rng.random(n) < p).astype(np.uint8), n_half, nhs)
    for i in range(n):                                               # one hit: counted while it is the record's own, cleared with the tail
        hits = np.zeros(n, np.uint8)
        hits[i] = 1
        check(H, L, hits, n_half, sorted({min(n, 380), min(i + 1, 380), min(i, 380)}))


def test_tail_mask_clears_what_it_cleared(H, L):
    """a record of nh k-mers beside a longer one: the wavefront's walk sets bits beyond nh in the record's last word (and above);
    after the decode tail_mask leaves k-mers (nw - 1) * 32 .. nh - 1 and nothing else"""
    n_half = 48
    hits = np.ones(8 * n_half, np.uint8)
    enc = list(encode(H, hits, n_half))
    for nh in range(1, 381):
        col = (C.c_uint32 * (MASKW + 1))(*enc)
        assert H.hb_count(col, nh, 1) == nh
        nw = L.sp_mask_words(nh)
        own = nh - (nw - 1) * 32
        assert L.sp_tail_mask(nh) == (0xFFFFFFFF << (32 - own)) & 0xFFFFFFFF
        assert col[nw - 1] == L.sp_tail_mask(nh) and all(col[w] == 0xFFFFFFFF for w in range(nw - 1)), nh


def test_a_second_decode_is_the_encoded_word_again(H, L):
    """why count_hits decodes under a flag: hit_decode is an involution, so the second round of a pass (HV == 2, after a candidate was
    struck) must find the flag off — decoding again would bring back upper = even ^ odd wherever the odd group has a hit"""
    rng = np.random.default_rng(77)
    for m in [0, 0xFFFFFFFF, 0x00010001, 0x80008000] + [int(x) for x in rng.integers(0, 1 << 32, size=2000)]:
        d = H.hb_decode(m)
        assert d == (m ^ (m << 16)) & 0xFFFFFFFF and H.hb_decode(d) == m
        assert (d == m) == ((m & 0xFFFF) == 0)                       # harmless only where the odd group has no hit
    n_half = 15                                                      # a 150 bp read, k = 31: 120 k-mers
    hits = (rng.random(8 * n_half) < 0.5).astype(np.uint8)
    enc = list(encode(H, hits, n_half))
    once, twice = (C.c_uint32 * (MASKW + 1))(*enc), (C.c_uint32 * (MASKW + 1))(*enc)
    H.hb_count(once, 120, 1)
    H.hb_count(twice, 120, 2)
    assert list(once)[:4] == image(L, hits, 120) and list(twice)[:4] != image(L, hits, 120)
    # the kernel's second round: words already decoded, a struck bit gone, NO decode — the image without that bit
    i = int(np.flatnonzero(hits[:120])[5])
    once[L.sp_kmer_word(i)] &= ~(1 << L.sp_kmer_bit(i))
    hits[i] = 0
    assert H.hb_count(once, 120, 0) == int(hits[:120].sum()) and list(once)[:4] == image(L, hits, 120)
