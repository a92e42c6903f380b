"""CPU tests of the seeding kernels' geometry (sylph_amd/csrc/seed_plan.h, compiled with g++ through tests/seed_plan_capi.cpp): how far
the read kernel's hash loop and windows read against what its LDS holds, where a k-mer's hit bit lands, the dealing by length, which
records belong to which block, the XCD dealing, the slot capacity and the layout of the block tables."""
import ctypes as C

import numpy as np
import pytest

from . import seed_plan_lib as SP


@pytest.fixture(scope="module")
def L():
    return SP.load()


@pytest.fixture(scope="module")
def K(L):
    return SP.constants()


def n_hashed(length, k, avx2):
    """device_common.h n_hashed_kmers for reads"""
    if length < k:
        return 0
    if not avx2:
        return length - k + 1
    return 0 if length < k + 1 else ((length - k + 1) // 4) * 4


def all_rt(K):
    lo, hi = K["RT_MIN"], K["RT_MAX"]
    mid = [int(x) // 16 * 16 for x in np.linspace(lo + 16, hi - 16, 64)]
    return sorted({lo, hi, *mid})


def test_constants_are_the_kernels(K):
    assert (K["RTPB"], K["RTPB_RAGGED"], K["RH"], K["MASKW"], K["NH_MAX"]) == (256, 512, 400, 12, 380)
    assert K["MASKW"] * 32 >= K["RH"] - 20 and K["TILE_WORDS"] == K["TPB"] * K["WPT"] and K["TILE_BASES"] == 16 * K["TILE_WORDS"]
    assert (K["TPB"] - 1) * K["WPT"] + 6 <= K["TILE_WORDS"] + K["HALO_WORDS"] and ((K["TILE_WORDS"] + K["HALO_WORDS"]) << 4) <= 1 << 16


def test_stream_window_holds_every_read_of_the_hash_loop(L, K):
    """check 1: every rt the plan can return, every rel of a record starting in the block, every nh_max up to RH - 21 + 1"""
    nh_top = K["RH"] - 21 + 1
    assert nh_top == K["NH_MAX"]
    for rt in all_rt(K):
        assert rt % 16 == 0
        out = (C.c_int64 * 4)()
        L.sp_window_max(rt, nh_top, out)
        loop_hi, win_hi, mate_hi, mate1_base = (int(x) for x in out)
        stream, lds = L.sp_stream_words(rt), L.sp_lds_words(rt)
        assert stream == (rt + 2 * K["RH"]) // 16 + 3 and lds == stream + K["RPAD"] == rt // 16 + 85, rt
        assert loop_hi == rt // 16 + 52 and loop_hi < lds, (rt, loop_hi, lds)          # the figure of the reference constants
        assert win_hi < stream and mate_hi < stream and mate1_base == 0, (rt, win_hi, mate_hi, stream, mate1_base)   # the farthest mate 1: stream base 0
        # what push_short_reads pays for is what the kernel indexes
        n_rec = 1000
        p = SP.plan(n_rec * (rt // 256), n_rec, 0, 200, 31)
        if p["rt"] == rt:
            assert p["lds_bytes"] == lds * 4


def test_mask_layout_bit_by_bit(L, K):
    """check 2: k-mer i at bit 31 - (i & 31) of word i >> 5 for every nh in 0..380, both lane counts; the tail mask clears exactly the
    bits at and beyond nh"""
    rng = np.random.default_rng(2)
    col = (C.c_uint32 * K["MASKW"])()
    for nh in range(0, 381):
        tpb = (256, 512)[nh & 1]
        slot = int(rng.integers(0, tpb))
        nh_max = min(380, nh + int(rng.integers(0, 40)))               # the wavefront's longest record: the lane walks its groups
        n_hit = 16 * ((L.sp_half_groups(nh_max) + 1) // 2) + 16
        hit = np.zeros(n_hit, np.uint8)
        hit[:nh] = rng.integers(0, 2, size=nh)
        hit[nh:] = 1                                                   # whatever lies beyond the record: never its own
        L.sp_mask_sim(hit.ctypes.data_as(C.POINTER(C.c_uint8)), nh_max, tpb, slot, 0xFFFFFFFF, col)
        words = [int(x) for x in col]
        n_stored = 8 * L.sp_half_groups(nh_max)
        for i in range(min(n_stored, K["MASKW"] * 32)):
            w, b = L.sp_kmer_word(i), L.sp_kmer_bit(i)
            assert (w, b) == (i >> 5, 31 - (i & 31))
            assert (words[w] >> b) & 1 == int(hit[i]), (nh, nh_max, i)
        nw = L.sp_mask_words(nh)
        assert nw == (nh + 31) // 32
        if nw:
            tail = L.sp_tail_mask(nh)
            words[nw - 1] &= tail
            own = [(words[i >> 5] >> (31 - (i & 31))) & 1 for i in range(nw * 32)]
            assert own[:nh] == [int(x) for x in hit[:nh]] and not any(own[nh:]), nh
            assert bin(tail).count("1") == nh - (nw - 1) * 32


def test_dealing_bins_rows_and_list(L, K):
    """check 3"""
    bins = [L.sp_deal_bin(nh) for nh in range(0, K["NH_MAX"] + 1)]
    assert min(bins) >= 0 and max(bins) <= 63 and bins[0] == 63
    assert all(a >= b for a, b in zip(bins, bins[1:]))                 # longer records never in a later bin: longest first
    for nh in range(0, K["NH_MAX"] + 1):
        hg = L.sp_half_groups(nh)
        assert hg == -(-nh // 8) and 63 - bins[nh] == hg
        rows = L.sp_rows_used(hg)
        direct = min(K["MASKW"], len({i >> 5 for i in range(hg * 8)}))  # mask words the hash loop writes for hg half-groups
        assert rows == direct and rows >= (nh + 31) // 32, nh
        for tpb in (256, 512):
            room = (K["MASKW"] - rows) * tpb
            for total in (0, 1, room - 1, room, room + 1, K["MASKW"] * tpb):
                if total >= 0:
                    assert bool(L.sp_listed(total, rows, tpb)) == (total <= room), (nh, tpb, total)
            assert room + rows * tpb <= K["MASKW"] * tpb and (K["MASKW"] * 32 - 1) << 10 | (tpb - 1) < 1 << 32


def random_offsets(rng, kind, n_rec):
    if kind == "tiny":
        lens = rng.integers(0, 30, size=n_rec)
    elif kind == "150":
        lens = np.full(n_rec, 150)
    elif kind == "400":
        lens = rng.integers(380, 401, size=n_rec)
    elif kind == "empty":
        lens = rng.integers(0, 200, size=n_rec) * rng.integers(0, 2, size=n_rec)
    else:                                                              # pairs: mates of 2 x 150 / trimmed
        lens = rng.integers(35, 152, size=n_rec)
    off = np.zeros(n_rec + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return off


@pytest.mark.parametrize("kind", ["tiny", "150", "400", "empty", "pairs"])
def test_every_record_belongs_to_one_block(L, K, kind):
    """check 4: random offset tables, bias 0..15 and the 2-bit phases (bias up to 15 * 4 + 3)"""
    rng = np.random.default_rng(len(kind))
    for bias in list(range(16)) + [16, 33, 63]:
        n_rec = int(rng.integers(1, 6000))
        off = random_offsets(rng, kind, n_rec)
        n_bases = int(off[-1])
        if n_bases == 0:
            continue
        for k, avx2, c in ((31, 1, 200), (21, 0, 1)):
            p = SP.plan(n_bases, n_rec, bias, c, k)
            rt, n_blk = p["rt"], p["n_blk"]
            assert K["RT_MIN"] <= rt <= K["RT_MAX"] and rt % 16 == 0 and n_blk * rt > n_bases + bias
            assert p["spill_cap"] == rt + K["RH"] and p["slot_cap"] == min(p["spill_cap"], (rt // c) + (rt // c) * 3 // 4 + 48)
            blk_rec, rel = SP.blocks(off, bias, rt, n_blk)
            assert blk_rec[0] == 0 and blk_rec[-1] == n_rec and (np.diff(blk_rec) >= 0).all()           # a partition of the records
            start = off[:-1].astype(np.int64) + bias
            blk_of = start // rt
            owner = np.repeat(np.arange(n_blk), np.diff(blk_rec))       # the block whose range [blk_rec[b], blk_rec[b + 1]) holds the record
            assert len(owner) == n_rec and np.array_equal(owner, blk_of)
            assert (rel >= K["RH"]).all() and (rel < K["RH"] + rt).all()
            assert np.array_equal(rel, start - (blk_of * rt - K["RH"]))
            lens = np.diff(off.astype(np.int64))
            nh = np.array([n_hashed(int(x), k, avx2) for x in lens])
            per_block = np.bincount(owner, weights=nh, minlength=n_blk)
            assert per_block.max() <= p["spill_cap"], (kind, bias, k)
            assert p["n_expect"] == max(0, n_bases - n_rec * (k - 1)) // c


def test_ragged_variant_and_clamps(L, K):
    p = SP.plan(150 * 1000, 1000)
    assert (p["tpb"], p["rt"]) == (256, 150 * 256)
    p = SP.plan(150 * 1000 + 1, 1000)                                  # ragged: 7 % lower
    assert p["tpb"] == 256 and p["rt"] == ((256 * 93 // 100 * 150001 // 1000) + 15) // 16 * 16
    p = SP.plan(100 * 1000 + 1, 1000, ragged_tpb_wanted=True)
    assert p["tpb"] == 512 and p["rt"] == ((512 * 93 // 100 * 100001 // 1000) + 15) // 16 * 16
    assert SP.plan(300 * 1000 + 1, 1000, ragged_tpb_wanted=True)["tpb"] == 256      # 512 such records do not fit the window
    assert SP.plan(10 * 1000, 1000)["rt"] == K["RT_MIN"] and SP.plan(400 * 1000, 1000)["rt"] == K["RT_MAX"]


def test_xcd_deal_is_a_bijection(L):
    """check 5"""
    for n in list(range(1, 301)) + [4096, 26001, 100003, (1 << 20) + 5]:
        m = L.sp_xcd_positions(n)
        assert m == 8 * -(-n // 8)
        i = np.arange(m, dtype=np.int64)
        img = (i & 7) * (m // 8) + (i >> 3)
        if n <= 300 or n == 26001:
            assert [L.sp_xcd_deal(int(x), n) for x in i[:600]] == img[:600].tolist()
        assert len(np.unique(img)) == m and img.min() == 0 and img.max() == m - 1          # a bijection of [0, m), so it covers [0, n)
        for pct in (0, 1, 5, 10, 50, 99):
            cut = L.sp_xcd_tail_cut(n, pct)
            assert cut % 8 == 0 and cut <= m
            assert cut == (m if (pct == 0 or m < 64) else (m * (100 - pct) // 100) & ~7)


def test_slot_capacity_in_both_kernels_shapes(L, K):
    """check 6"""
    for c in (1, 2, 3, 20, 200, 1000):
        for full, per in ((K["TILE_BASES"], K["TILE_BASES"]), *((rt + K["RH"], rt) for rt in (K["RT_MIN"], 38400, 35712, K["RT_MAX"]))):
            expect = per // c
            got = L.sp_slot_capacity(full, expect)
            assert got == min(full, expect + expect * 3 // 4 + 48) and got <= full


def test_slot_meta_is_the_layout_the_replay_and_the_filter_read(L):
    """check 7: the hand expressions a10.hip and replay_lds.hip carried, in 32-bit words from the buffer's start"""
    state_bytes = 4 + 4 + 256 * 4                                        # ReadsState: long_record, SpillState{n_tiles, tiles[256]}
    for n_blk in (1, 2, 7, 26041, 1 << 20):
        out = (C.c_uint64 * 6)()
        L.sp_slot_meta(n_blk, state_bytes, out)
        blk_rec, blk_count, spill_slot, blk_off, state, nbytes = (int(x) for x in out)
        assert blk_rec == 0
        assert blk_count == (n_blk + 1)                                  # a10.hip:587 and replay_lds.hip:427: as<uint32_t>() + (n_blk + 1)
        assert state == (n_blk + 1) * 4                                  # replay_lds.hip:303: as<uint32_t>() + (size_t)(n_blk + 1) * 4
        assert spill_slot == 2 * (n_blk + 1) and blk_off == 3 * (n_blk + 1)
        assert blk_off + n_blk + 1 == state                              # the total blk_off[n_blk] and the two flag words: one 12-byte copy
        assert nbytes == (n_blk + 1) * 4 * 4 + state_bytes + 16          # reads.hip: what push_short_reads reserved
