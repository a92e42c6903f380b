"""CPU tests of the replay's bucket map (sylph_amd/csrc/replay_plan.h, the very header the partition and replay kernels include, compiled
with g++ through tests/replay_plan_capi.cpp): the map finish_bucketed derives from a sample's size, the bucket of a key and its two
inverses, and the sub-range of a key inside its bucket — bucket by bucket over sampling rates, sample sizes and bucket targets — and the
Python copy of the map that tests/test_gpu_replay_lane.py states its preconditions with (helpers.bucket_roads)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from .helpers import bucket_roads

HERE = os.path.dirname(os.path.abspath(__file__))
N_CFG = 4


class BucketMap(C.Structure):
    _fields_ = [("sh", C.c_int), ("mult", C.c_uint32), ("B", C.c_uint32), ("composite", C.c_int), ("range_hs", C.c_uint32),
                ("sub_mult", C.c_uint32 * N_CFG), ("sub_width", C.c_uint32 * N_CFG), ("rank_bits", C.c_int * N_CFG), ("inv_mult", C.c_uint64)]


@pytest.fixture(scope="module")
def L():
    out = os.path.join(tempfile.gettempdir(), f"sylph_replay_plan_{os.getuid()}.so")
    src = os.path.join(HERE, "replay_plan_capi.cpp")
    hdr = os.path.join(HERE, "..", "sylph_amd", "csrc", "replay_plan.h")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, src])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    lib.rp_map_bytes.restype = C.c_uint32
    lib.rp_constants.argtypes = [C.POINTER(C.c_int32)]
    lib.rp_make_bucket_map.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(BucketMap)]
    lib.rp_bucket_lows.argtypes = [C.POINTER(BucketMap), u32p, C.c_uint64, u64p, u64p]
    lib.rp_bucket_of_keys.argtypes = [C.POINTER(BucketMap), u32p, C.c_uint64, u32p]
    lib.rp_sub_ranges.argtypes = [u32p, C.c_uint64, C.c_uint32, C.c_uint32, u32p]
    assert lib.rp_map_bytes() == C.sizeof(BucketMap)
    return lib


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32 if a.dtype == np.uint32 else C.c_uint64))


def make_map(L, c, n_all, target, max_index=None):
    bm = BucketMap()
    L.rp_make_bucket_map(c, n_all, target, n_all if max_index is None else max_index, C.byref(bm))
    return bm


def bucket_lows(L, bm, b):
    b = u32(b)
    lo_key, lo_hash = np.zeros(len(b), np.uint64), np.zeros(len(b), np.uint64)
    L.rp_bucket_lows(C.byref(bm), ptr(b), len(b), ptr(lo_key), ptr(lo_hash))
    return lo_key, lo_hash


def bucket_of_keys(L, bm, keys):
    keys = u32(keys)
    out = np.zeros(len(keys), np.uint32)
    L.rp_bucket_of_keys(C.byref(bm), ptr(keys), len(keys), ptr(out))
    return out.astype(np.int64)


def sub_ranges(L, res, sub_mult, cap):
    res = u32(res)
    out = np.zeros(len(res), np.uint32)
    L.rp_sub_ranges(ptr(res), len(res), sub_mult, cap, ptr(out))
    return out.astype(np.int64)


def constants(L):
    v = (C.c_int32 * (8 + N_CFG))()
    L.rp_constants(v)
    names = ("CAP_SMALL", "CAP_MID", "CAP_LARGE", "LANE_CAP", "LANE_CFG", "N_CFG", "IDX_BITS", "SEG_LIMIT")
    return dict(zip(names, v[:8]), caps=list(v[8:]))


def test_configuration_indices_and_capacities_agree(L):
    k = constants(L)
    assert k["N_CFG"] == N_CFG and k["caps"] == [k["CAP_SMALL"], k["CAP_MID"], k["CAP_LARGE"], k["LANE_CAP"]]
    assert k["caps"][k["LANE_CFG"]] == k["LANE_CAP"] == 128 and (k["CAP_SMALL"], k["CAP_MID"], k["CAP_LARGE"]) == (256, 512, 1024)
    assert k["CAP_LARGE"] <= 1 << k["IDX_BITS"] and k["SEG_LIMIT"] == 96


C_VALUES = (2, 3, 7, 20, 100, 200, 1000)
OCCURRENCES = (1, 95, 96, 300, 5000, 4 * 10**6, 4 * 10**8, 4 * 10**9)
TARGETS = (16, 64, 96, 128, 256)


@pytest.mark.parametrize("c", C_VALUES)
def test_bucket_map_bucket_by_bucket(L, c):
    caps = constants(L)["caps"]
    rng = np.random.default_rng(c)
    thr = (2**64 - 1) // c
    checked = 0
    for n_all in OCCURRENCES:
        for target in TARGETS:
            bm = make_map(L, c, n_all, target)
            B, sh, at = int(bm.B), int(bm.sh), (c, n_all, target)
            assert B == min(max(1, n_all // target), 1 << 24) and int(bm.mult) >= 1, at
            key_max = (thr - 1) >> sh                                # hashes are below thr
            assert key_max < 2**32, at
            if B <= 2000:
                b = np.arange(B, dtype=np.int64)
            else:
                b = np.unique(np.concatenate([[0, 1, 2, B - 2, B - 1], rng.integers(0, B, size=2000)])).astype(np.int64)
            lo_key, lo_hash = bucket_lows(L, bm, b)
            # the division-free low is the low
            assert np.array_equal(lo_key << np.uint64(sh), lo_hash), at
            lo = lo_key.astype(object)                                # (exact integers from here on: a low may be 2^32)
            live = np.array([int(v) <= key_max for v in lo])          # buckets that hold a key at all
            assert live[0] and int(lo[0]) == 0, at
            b, lo = b[live], np.array([int(v) for v in lo[live]], dtype=np.int64)
            # the low is the first key of its bucket
            assert np.array_equal(bucket_of_keys(L, bm, lo), b), at
            assert np.array_equal(bucket_of_keys(L, bm, lo[b > 0] - 1), b[b > 0] - 1), at
            # the last key of bucket b: the one before the next bucket's low, the highest key for the last bucket that holds one
            nxt, _ = bucket_lows(L, bm, np.minimum(b + 1, B - 1))
            nxt = np.array([int(v) for v in nxt.astype(object)], dtype=np.int64)
            hi = np.where((b + 1 < B) & (nxt <= key_max), nxt - 1, key_max)
            assert np.array_equal(bucket_of_keys(L, bm, hi), b), at
            # every key of a bucket lies less than range_hs above its low (range_hs = ceil(2^32 / mult) + 1; the field is 32 bits wide
            # and holds 2^32 - 1 where the width itself is 2^32 + 1: mult = 1, the single bucket of the smallest samples)
            range_hs = (2**32 + int(bm.mult) - 1) // int(bm.mult) + 1
            assert int(bm.range_hs) == min(range_hs, 0xFFFFFFFF), at
            d_max = hi - lo
            assert d_max.min() >= 0 and d_max.max() < range_hs, at
            # sub-ranges of every configuration at distances 0 <= random <= half ... max (sorted per bucket)
            d_rnd = (rng.random(len(b)) * (d_max + 1)).astype(np.int64).clip(0, d_max)
            dist = np.sort(np.stack([np.zeros_like(d_max), d_max // 2, d_rnd, d_max]), axis=0)
            for i, cap in enumerate(caps):
                sub = np.stack([sub_ranges(L, d, int(bm.sub_mult[i]), cap) for d in dist])
                assert sub.min() >= 0 and sub.max() < cap, (at, i)
                assert (np.diff(sub, axis=0) >= 0).all(), (at, i)                    # monotone
                res = dist - sub * int(bm.sub_width[i])
                assert res.min() >= 0, (at, i)                                       # the residue is never negative
                if bm.rank_bits[i] > 0:
                    assert bm.composite, (at, i)
                    # (hash - lowest hash of the sub-range) << rank_bits: the hash's bits below sh ride along
                    top = ((int(res.max()) + 1) << sh) - 1
                    assert top.bit_length() + int(bm.rank_bits[i]) <= 64, (at, i)
                    assert int(bm.rank_bits[i]) == max(1, n_all.bit_length()), (at, i)     # room for every index
            checked += len(b)
    print(f"c = {c}: {checked} buckets checked")
    assert checked > 1000


LANE_TEST_MAPS = ((20, 64), (20, 124), (20, 256), (7, 16), (10, 64), (3, 128))      # (c, bucket_target) of test_gpu_replay_lane.py


@pytest.mark.parametrize("c,target", LANE_TEST_MAPS)
def test_bucket_roads_is_the_map(L, c, target):
    rng = np.random.default_rng(1000 * c + target)
    for n in (3000, 150000):                                        # (c = 3: not composite / composite)
        hashes = rng.integers(0, (2**64 - 1) // c, size=n, dtype=np.uint64)
        roads = bucket_roads(hashes, c, target)
        bm = make_map(L, c, n, target)
        assert roads["B"] == bm.B and bool(roads["composite"]) == bool(bm.composite), (c, target, n)
        bucket = bucket_of_keys(L, bm, hashes >> np.uint64(bm.sh))
        assert np.array_equal(roads["bucket"], bucket) and np.array_equal(roads["n"], np.bincount(bucket, minlength=int(bm.B))), (c, target, n)
        if bm.composite:        # the fullest sub-range of the body that runs each bucket, from the header's arithmetic
            lo_key, _ = bucket_lows(L, bm, np.arange(bm.B))
            res = (hashes >> np.uint64(bm.sh)) - lo_key[bucket]
            fill = np.zeros(int(bm.B), dtype=np.int64)
            for cfg, cap in ((3, 128), (0, 256)):
                of_cap = (roads["n"][bucket] <= 128) == (cap == 128)
                sub = sub_ranges(L, res, int(bm.sub_mult[cfg]), cap)
                fill = np.maximum(fill, np.bincount((bucket * 256 + sub)[of_cap], minlength=int(bm.B) * 256).reshape(-1, 256).max(axis=1))
            assert np.array_equal(roads["fill"], fill), (c, target, n)
