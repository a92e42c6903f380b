"""CPU tests of what a lane of the read kernel carries through its hash loop and of the arithmetic that took the place of 64-bit work
around it (sylph_amd/csrc/seed_plan.h, compiled with g++ through tests/pass_state_capi.cpp):

  * emission_lane — three compares against len4, 2 len4, 3 len4 — is i / len4 for EVERY record the read kernel can hold (nh <= NH_MAX, a
    multiple of 4, every i < nh) and for a sample of large nh (the position kernel takes long records through the same function);
    emission_rank built on it is the reference's emission order, and position order without the AVX2-compatible rule;
  * rel_bias + record_rel32 — one 32-bit add on an offset's low word — is record_rel's 64-bit sum and difference, for offsets up to
    2^32 - 1 (and beyond), every bias 0..63, and blocks at the first and at the last a0 of a batch, at both clamps of the block size and
    the flagship's;
  * MarkerBases is the rule publish_markers applied to 64-bit offsets (sketch.rs:625-688), and bb = 0 says "no markers" of no marked
    record;
  * stream_word_range is the per-word test a0 + 16 ci in [0, n_al) of the first and last blocks' loads, block_starts_inside the sign of
    block_a0."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

from . import seed_plan_lib as SP

HERE = os.path.dirname(os.path.abspath(__file__))
U32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def P():
    src = os.path.join(HERE, "pass_state_capi.cpp")
    hdr = os.path.join(HERE, "..", "sylph_amd", "csrc", "seed_plan.h")
    key = hashlib.sha256(open(src, "rb").read() + open(hdr, "rb").read()).hexdigest()[:16]
    out = os.path.join(tempfile.gettempdir(), f"sylph_pass_state_{os.getuid()}_{key}.so")
    if not os.path.exists(out):
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, src])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    sig = {"ps_emission_lane": (C.c_uint32, [C.c_uint32, C.c_uint32]), "ps_emission_rank": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_int]),
           "ps_emission_mismatches": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32]),
           "ps_n_hashed_kmers": (C.c_uint64, [C.c_uint64, C.c_uint32, C.c_int, C.c_int]),
           "ps_record_rel": (C.c_uint32, [C.c_uint64, C.c_uint32, C.c_int64]), "ps_rel_bias": (C.c_uint32, [C.c_uint32, C.c_int64]),
           "ps_record_rel32": (C.c_uint32, [C.c_uint64, C.c_uint32]), "ps_rel_mismatches": (C.c_uint64, [u64p, C.c_uint64, C.c_uint32, C.c_int64]),
           "ps_single_marker_bases": (None, [C.c_uint32, C.c_uint32, u32p]),
           "ps_pair_marker_bases": (None, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u32p]),
           "ps_stream_word_range": (None, [C.c_int64, C.c_uint64, C.c_uint32, u32p]), "ps_block_starts_inside": (C.c_int, [C.c_uint32]),
           "ps_block_a0": (C.c_int64, [C.c_uint32, C.c_uint32]), "ps_stream_words": (C.c_uint32, [C.c_uint32])}
    for name, (res, args) in sig.items():
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    return lib


@pytest.fixture(scope="module")
def K():
    return SP.constants()


def test_the_compare_form_is_the_division_for_every_record_of_the_read_kernel(P, K):
    assert K["NH_MAX"] == 380
    checked = 0
    for nh in range(4, K["NH_MAX"] + 1, 4):
        assert P.ps_emission_mismatches(nh, 0, nh) == 0, nh
        checked += nh
    assert checked == sum(range(4, 381, 4))
    # the edges by hand: the first and the last k-mer of every quarter
    for nh in (4, 8, 120, 380):
        len4 = nh // 4
        for q in range(4):
            for i in (q * len4, (q + 1) * len4 - 1):
                assert P.ps_emission_lane(i, len4) == q
                assert P.ps_emission_rank(i, nh, 1) == (i - q * len4) * 4 + q
                assert P.ps_emission_rank(i, nh, 0) == i
    # fewer than four k-mers, or the scalar rule: position order
    for nh in range(0, 4):
        for i in range(nh):
            assert P.ps_emission_rank(i, nh, 1) == i


def test_the_compare_form_on_long_records(P):
    """the position kernel's records: nh up to 2^32 - 4 (3 len4 must not wrap), every quarter's edges and a random sample"""
    rng = np.random.default_rng(1500)
    nhs = [4 * int(x) for x in rng.integers(1, 1 << 30, size=200)] + [U32 - 3, 1 << 31, (1 << 31) + 4, 4 * 0x2AAAAAAB, 1000, 100000, 12345678 * 4]
    for nh in nhs:
        assert nh % 4 == 0 and 4 <= nh <= U32 - 3
        len4 = nh // 4
        for q in range(4):
            for i in (q * len4, q * len4 + 1, (q + 1) * len4 - 1):
                if i < nh:
                    assert P.ps_emission_lane(i, len4) == i // len4 == q, (nh, i)
                    assert P.ps_emission_rank(i, nh, 1) == (i - q * len4) * 4 + q, (nh, i)
        for i in rng.integers(0, nh, size=50).tolist():
            assert P.ps_emission_lane(i, len4) == i // len4, (nh, i)
        lo = int(rng.integers(0, nh))
        assert P.ps_emission_mismatches(nh, lo, 5000) == 0, (nh, lo)


def test_n_hashed_kmers_is_what_it_was(P):
    for k in (21, 31):
        for L in list(range(0, 500)) + [10**6 + 3, (1 << 33) + 2]:
            scalar = L - k + 1 if L >= k else 0
            assert P.ps_n_hashed_kmers(L, k, 0, 0) == scalar
            assert P.ps_n_hashed_kmers(L, k, 1, 0) == (scalar // 4 * 4 if L >= k + 1 else 0)
            assert P.ps_n_hashed_kmers(L, k, 1, 1) == (scalar // 4 * 4 if L >= 2 * k else 0)


def batch_blocks(P, K, n_al, rt):
    """(blk, a0) of the first, the second, a middle and the last block of a batch with n_al aligned coordinates"""
    n_blk = n_al // rt + 1
    return [(b, P.ps_block_a0(b, rt)) for b in sorted({0, 1, n_blk // 2, n_blk - 2, n_blk - 1}) if 0 <= b < n_blk]


@pytest.mark.parametrize("rt", [4096, 38400, 65536])
def test_the_32_bit_step_is_record_rel(P, K, rt):
    """offsets up to 2^32 - 1 — a GPU test cannot reach them at small size — and past 2^32; bias 0..63; the blocks at both ends of the batch"""
    RH = K["RH"]
    assert K["RT_MIN"] <= rt <= K["RT_MAX"]
    rng = np.random.default_rng(rt)
    for top in (U32, (1 << 32) + 5 * rt + 17, (1 << 40) + 3):          # the batch's last offset
        for bias in range(64):
            n_al = top + bias
            for blk, a0 in batch_blocks(P, K, n_al, rt):
                assert a0 == blk * rt - RH and a0 % 16 == 0
                rb = P.ps_rel_bias(bias, a0)
                # coordinates of the block's own records, [blk rt, (blk + 1) rt), and of a mate 1 up to RH in front; offsets = coordinate - bias
                lo, hi = max(blk * rt - RH, bias), min((blk + 1) * rt, n_al + 1)
                if lo >= hi:
                    continue
                coords = np.unique(np.concatenate([np.array([lo, min(lo + 1, hi - 1), max(blk * rt, lo), hi - 1], np.uint64),
                                                   rng.integers(lo, hi, size=40).astype(np.uint64)]))
                starts = (coords - np.uint64(bias)).astype(np.uint64)
                assert P.ps_rel_mismatches(starts.ctypes.data_as(C.POINTER(C.c_uint64)), len(starts), bias, a0) == 0, (top, bias, blk)
                for s, co in zip(starts.tolist()[:6], coords.tolist()[:6]):
                    rel = P.ps_record_rel32(s, rb)
                    assert rel == P.ps_record_rel(s, bias, a0) == co - a0, (top, bias, blk, s)      # the value itself: a stream base inside the block's window
                    assert 0 <= rel < RH + rt
    # the largest offset a 32-bit word holds, at the last block that can hold it
    for bias in (0, 1, 15, 63):
        blk = (U32 + bias) // rt
        a0 = P.ps_block_a0(blk, rt)
        assert P.ps_record_rel32(U32, P.ps_rel_bias(bias, a0)) == P.ps_record_rel(U32, bias, a0) == U32 + bias - a0


def old_markers(P, paired, start, s1, s2, e2, L, bias, a0):
    """publish_markers as it was, on 64-bit offsets: (has, ba, bb)"""
    if not paired:
        if 66 <= L <= 400:
            rel = P.ps_record_rel(start, bias, a0)
            return 1, rel, rel + L // 2
        return 0, 0, 0
    if s2 - s1 >= 33 and e2 - s2 >= 33:
        return 1, P.ps_record_rel(s1, bias, a0), P.ps_record_rel(s2, bias, a0)
    return 0, 0, 0


def test_marker_bases_are_the_rule_on_64_bit_offsets(P, K):
    RH, rt = K["RH"], 38400
    out = (C.c_uint32 * 2)()
    rng = np.random.default_rng(66)
    lens = [0, 1, 30, 31, 32, 33, 34, 65, 66, 67, 150, 151, 399, 400]
    for bias in (0, 5, 63):
        for blk in (0, 1, (U32 + bias) // rt):
            a0 = P.ps_block_a0(blk, rt)
            rb = P.ps_rel_bias(bias, a0)
            base = max(blk * rt, bias) - bias                              # offset of a record on the block's first coordinate (or the batch's first)
            for start in (base, base + 1, base + int(rng.integers(2, rt - 801))):
                if start + 800 > U32:
                    start = U32 - 800
                for L in lens:                                             # single reads
                    has, ba, bb = old_markers(P, False, start, 0, 0, 0, L, bias, a0)
                    rel = P.ps_record_rel32(start, rb)
                    P.ps_single_marker_bases(rel, L, out)
                    assert (out[0], out[1]) == (ba, bb) and (out[1] != 0) == bool(has), (bias, blk, start, L)
                for L1 in lens:                                            # pairs: the lane may be either mate, the bases are the pair's
                    for L2 in lens:
                        s1, s2, e2 = start, start + L1, start + L1 + L2
                        has, ba, bb = old_markers(P, True, 0, s1, s2, e2, 0, bias, a0)
                        P.ps_pair_marker_bases(P.ps_record_rel32(s1, rb), P.ps_record_rel32(s2, rb), L1, L2, out)
                        assert (out[0], out[1]) == (ba, bb) and (out[1] != 0) == bool(has), (bias, blk, start, L1, L2)
    # a mate 2 on a block's first coordinate, its mate 1 in the halo: ba may be anything from 0 on, bb is never 0
    a0 = P.ps_block_a0(3, rt)
    rb = P.ps_rel_bias(0, a0)
    for L1 in (33, 150, 400):
        s2 = 3 * rt
        P.ps_pair_marker_bases(P.ps_record_rel32(s2 - L1, rb), P.ps_record_rel32(s2, rb), L1, 150, out)
        assert (out[0], out[1]) == (RH - L1, RH)


def test_stream_word_range_is_the_per_word_test(P, K):
    for rt in (K["RT_MIN"], 38400, K["RT_MAX"]):
        n_words = P.ps_stream_words(rt)
        out = (C.c_uint32 * 2)()
        for n_al in (1, 15, 16, 17, 399, 400, 401, rt - 1, rt, rt + 1, 3 * rt + 77, 10 * rt, 10 * rt + 16 * 5 + 3, U32 + 63, (1 << 33) + 9):
            n_blk = n_al // rt + 1
            for blk in sorted({0, 1, 2, n_blk - 2, n_blk - 1} & set(range(n_blk))):
                a0 = P.ps_block_a0(blk, rt)
                assert P.ps_block_starts_inside(blk) == (a0 >= 0)
                P.ps_stream_word_range(a0, n_al, n_words, out)
                ci = np.arange(n_words, dtype=np.int64)
                a = a0 + 16 * ci
                inside = (a >= 0) & (a < n_al)
                assert np.array_equal(inside, (ci >= out[0]) & (ci < out[1])), (rt, n_al, blk)
                assert out[0] <= n_words and out[1] <= n_words
