"""The seeding kernels' geometry (sylph_amd/csrc/seed_plan.h, the very header the kernels include) as a ctypes library, compiled with g++
through tests/seed_plan_capi.cpp: tests/test_seed_plan.py checks it, tests/test_gpu_reads_blocks.py places its records with it."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CONSTANTS = ("RTPB", "RTPB_RAGGED", "RT_MIN", "RT_MAX", "RH", "RPAD", "MASKW", "OFFS_256", "NH_MAX", "TPB", "WPT", "TILE_WORDS", "TILE_BASES",
             "HALO_WORDS", "LIST_CAP", "STAGE_CAP", "FLUSH_AT")
PLAN_FIELDS = ("tpb", "rt", "n_blk", "slot_cap", "spill_cap", "lds_bytes", "n_expect")
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    src = os.path.join(HERE, "seed_plan_capi.cpp")
    hdr = os.path.join(HERE, "..", "sylph_amd", "csrc", "seed_plan.h")
    key = hashlib.sha256(open(src, "rb").read() + open(hdr, "rb").read()).hexdigest()[:16]      # two checkouts on one machine: two libraries
    out = os.path.join(tempfile.gettempdir(), f"sylph_seed_plan_{os.getuid()}_{key}.so")
    if not os.path.exists(out):
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, src])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    lib.sp_constants.argtypes = [C.POINTER(C.c_int32)]
    lib.sp_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, u64p]
    lib.sp_slot_capacity.argtypes = [C.c_uint64, C.c_uint64]
    lib.sp_window_max.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_int64)]
    lib.sp_mask_sim.argtypes = [u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u32p]
    lib.sp_blocks.argtypes = [u64p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, u64p, u32p]
    lib.sp_block_a0.argtypes = [C.c_uint32, C.c_uint32]
    lib.sp_block_a0.restype = C.c_int64
    lib.sp_slot_meta.argtypes = [C.c_uint32, C.c_uint64, u64p]
    for name in ("sp_slot_capacity", "sp_stream_words", "sp_lds_words", "sp_kmer_word", "sp_kmer_bit", "sp_mask_words", "sp_tail_mask", "sp_half_groups",
                 "sp_deal_bin", "sp_rows_used", "sp_xcd_deal", "sp_xcd_positions", "sp_xcd_tail_cut"):
        getattr(lib, name).restype = C.c_uint32
        if name not in ("sp_slot_capacity",):
            getattr(lib, name).argtypes = [C.c_uint32] * (2 if name in ("sp_xcd_deal", "sp_xcd_tail_cut") else 1)
    lib.sp_listed.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    _lib = lib
    return lib


def constants():
    v = (C.c_int32 * len(CONSTANTS))()
    load().sp_constants(v)
    return dict(zip(CONSTANTS, v))


def plan(n_bases, n_records, bias=0, c=200, k=31, ragged_tpb_wanted=False):
    """reads_block_plan: what push_short_reads cuts a batch into"""
    v = (C.c_uint64 * len(PLAN_FIELDS))()
    load().sp_plan(n_bases, n_records, bias, c, k, int(ragged_tpb_wanted), v)
    return dict(zip(PLAN_FIELDS, (int(x) for x in v)))


def blocks(off, bias, rt, n_blk):
    """-> (blk_rec[n_blk + 1]: the first record of every block, rel[n_rec]: every record's stream base in its block)"""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n_rec = len(off) - 1
    blk_rec, rel = np.zeros(n_blk + 1, np.uint64), np.zeros(max(n_rec, 1), np.uint32)
    load().sp_blocks(off.ctypes.data_as(C.POINTER(C.c_uint64)), n_rec, bias, rt, n_blk, blk_rec.ctypes.data_as(C.POINTER(C.c_uint64)),
                     rel.ctypes.data_as(C.POINTER(C.c_uint32)))
    return blk_rec.astype(np.int64), rel[:n_rec].astype(np.int64)
