"""CPU tests of a pre-sketched sample's table arithmetic (sylph_amd/csrc/sylsp_plan.h, the very header sylsp.hip includes, compiled
with g++ through tests/sylsp_plan_capi.cpp) against numpy: the tile geometry at every dword phase of the entry base, the entry
decode, the order rule across tile boundaries, the keep rule of the general road (stable argsort by key, last of each run) — a
lane-by-lane replay of the unpack kernel included — the host's read_sylsp_header against read_sylsp, and the stand-alone
sanitizer run."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from .helpers import build_path
from .sylsp_tables import CASE_KINDS, SIZES, entries_case, model_table, pack_entries

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = os.path.join(HERE, "..", "sylph_amd", "csrc", "sylsp_plan.h")
SRC = os.path.join(HERE, "sylsp_plan_capi.cpp")
u64, u32, i32, vp = C.c_uint64, C.c_uint32, C.c_int, C.c_void_p
T = 256


@pytest.fixture(scope="module")
def L():
    out, stale = build_path("sylph_sylsp_plan", [SRC, HDR], ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, SRC])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    lib.sp_constants.argtypes = [vp]
    lib.sp_base_phase.restype = u32
    lib.sp_base_phase.argtypes = [u64]
    lib.sp_n_tiles.restype = u32
    lib.sp_n_tiles.argtypes = [u64]
    lib.sp_tile_entries.restype = u32
    lib.sp_tile_entries.argtypes = [u32, u64]
    lib.sp_tile_window.argtypes = [u32, u64, u32, vp]
    lib.sp_lane_lds_dword.restype = u32
    lib.sp_lane_lds_dword.argtypes = [u32, u32]
    lib.sp_prev_key_dword.restype = u64
    lib.sp_prev_key_dword.argtypes = [u64]
    lib.sp_entry_from_words.argtypes = [u32, u32, u32, vp, vp]
    lib.sp_breaks_order.argtypes = [u64, u64, u64]
    lib.sp_last_of_run.argtypes = [u64, u64, u64, u64]
    lib.sp_model_unpack.restype = i32
    lib.sp_model_unpack.argtypes = [vp, u64, u32, vp, vp]
    lib.sp_model_table.restype = u64
    lib.sp_model_table.argtypes = [vp, vp, u64, vp, vp]
    k = np.zeros(9, dtype=np.uint64)
    lib.sp_constants(k.ctypes.data)
    assert [int(v) for v in k] == [12, 3, 8, 2**31, 16, T, 3 * T, 193, 772]
    return lib


def test_sizes_of_the_shared_cases_follow_the_tile():
    assert SIZES[:7] == [0, 1, 2, T - 1, T, T + 1, 2 * T + 1]


def test_tile_geometry_at_every_phase(L):
    """Every tile's window is 16-byte aligned, covers exactly its entries' dwords plus the phase in front, reaches at most 12 bytes
    either side of the stream, and fits the LDS array; a lane's three dwords are its entry's."""
    o = np.zeros(2, dtype=np.int64)
    for phase in range(4):
        for addr16 in (0, 0x7F00_0000_1000):
            assert L.sp_base_phase(addr16 + 4 * phase) == phase
        for n in SIZES + [3 * T, 2**31 - 1]:
            nt = L.sp_n_tiles(n)
            assert nt == -(-n // T)
            tiles = range(nt) if nt <= 8 else [0, 1, nt - 2, nt - 1]
            for t in tiles:
                m = L.sp_tile_entries(t, n)
                assert m == min(T, n - t * T) and m >= 1
                L.sp_tile_window(t, n, phase, o.ctypes.data)
                first, n_vecs = int(o[0]), int(o[1])
                assert (first + phase) % 4 == 0 and first == 3 * T * t - phase          # aligned; `phase` dwords in front
                assert first >= -3 and first + 4 * n_vecs <= 3 * n + 3                  # at most 12 bytes either side of the stream
                assert 4 * n_vecs >= phase + 3 * m > 4 * (n_vecs - 1) and n_vecs <= 193 <= T
                for lane in {0, min(1, m - 1), m // 2, m - 1}:
                    at = L.sp_lane_lds_dword(lane, phase)
                    assert first + at == 3 * (t * T + lane) and at + 2 < 4 * n_vecs
    assert L.sp_prev_key_dword(1) == 0 and L.sp_prev_key_dword(T) == 3 * (T - 1) and L.sp_prev_key_dword(2**31 - 1) == 3 * (2**31 - 2)


def test_entry_decode_and_rules(L):
    k, c = u64(0), u32(0)
    for kmer, count in ((0, 0), (2**64 - 1, 2**32 - 1), (0x0123456789ABCDEF, 7), (2**32, 1), (2**32 - 1, 2**31)):
        w = struct.unpack("<III", struct.pack("<QI", kmer, count))
        L.sp_entry_from_words(w[0], w[1], w[2], C.byref(k), C.byref(c))
        assert (k.value, c.value) == (kmer, count)
    M = 2**64 - 1
    assert not L.sp_breaks_order(0, M, 0)                                  # entry 0 never breaks the order
    assert L.sp_breaks_order(1, 5, 5) and L.sp_breaks_order(1, 5, 4) and not L.sp_breaks_order(1, 5, 6)
    assert L.sp_breaks_order(T, M, M) and not L.sp_breaks_order(T, M - 1, M) and L.sp_breaks_order(7, 2**63, 2**63 - 1)   # unsigned compare
    assert L.sp_last_of_run(4, 5, 9, 9) and L.sp_last_of_run(0, 1, 0, 0)   # the last entry: whatever "next" holds
    assert not L.sp_last_of_run(3, 5, 9, 9) and L.sp_last_of_run(3, 5, 9, 10) and L.sp_last_of_run(0, 2, M, 0)


def run_model(L, kmers, counts, phase):
    n = len(kmers)
    raw = pack_entries(kmers, counts)
    uk, uc = np.zeros(max(1, n), dtype=np.uint64), np.zeros(max(1, n), dtype=np.uint32)
    flag = L.sp_model_unpack(raw.ctypes.data, n, phase, uk.ctypes.data, uc.ctypes.data)
    assert flag in (0, 1), flag                                            # negative: a load or an index left its bounds
    assert np.array_equal(uk[:n], kmers) and np.array_equal(uc[:n], counts)
    if not flag:
        return flag, uk[:n], uc[:n]
    tk, tc = np.zeros(max(1, n), dtype=np.uint64), np.zeros(max(1, n), dtype=np.uint32)
    m = L.sp_model_table(uk.ctypes.data, uc.ctypes.data, n, tk.ctypes.data, tc.ctypes.data)
    return flag, tk[:m], tc[:m]


@pytest.mark.parametrize("phase", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", CASE_KINDS)
def test_replayed_kernel_against_numpy(L, kind, phase):
    for n in SIZES:
        kmers, counts = entries_case(kind, n, seed=phase)
        want_k, want_c = model_table(kmers, counts)
        flag, got_k, got_c = run_model(L, kmers, counts, phase)
        ascending = n < 2 or bool((kmers[1:] > kmers[:-1]).all())
        assert bool(flag) == (not ascending), (kind, n)
        assert np.array_equal(got_k, want_k) and np.array_equal(got_c, want_c), (kind, n)


@pytest.mark.parametrize("phase", [0, 3])
def test_break_exactly_at_a_tile_boundary(L, phase):
    """Ascending inside every tile; only entry T (the first of tile 1) is not above its predecessor — the comparison must cross the
    boundary; with equality there, and with a smaller key."""
    for n in (T + 1, 2 * T + 1):
        base = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(1000)
        counts = np.arange(n, dtype=np.uint32)
        for below in (0, 1):                                               # entry T equal to its predecessor / one below it
            kmers = base.copy()
            kmers[T] = kmers[T - 1] - np.uint64(below)
            breaks = np.nonzero(kmers[1:] <= kmers[:-1])[0] + 1
            assert breaks.tolist() == [T]                                  # there and nowhere else
            flag, got_k, got_c = run_model(L, kmers, counts, phase)
            want_k, want_c = model_table(kmers, counts)
            assert flag == 1 and np.array_equal(got_k, want_k) and np.array_equal(got_c, want_c)
            if below == 0:
                assert len(got_k) == n - 1 and T - 1 not in got_c.tolist() and T in got_c.tolist()   # the repeated key kept its LAST count
            else:
                assert len(got_k) == n and got_c[T - 1:T + 1].tolist() == [T, T - 1]
        assert run_model(L, base, counts, phase)[0] == 0                   # the same shape without the break: flag clear


def test_duplicate_whose_last_count_is_zero(L):
    kmers = np.array([50, 7, 50, 9, 50, 7], dtype=np.uint64)
    counts = np.array([3, 1, 4, 2, 0, 5], dtype=np.uint32)
    flag, got_k, got_c = run_model(L, kmers, counts, 2)
    assert flag == 1 and got_k.tolist() == [7, 9, 50] and got_c.tolist() == [5, 2, 0]   # the kept count of 0 stays in the table


# ---- the host's reader -------------------------------------------------------------------------------------------------------

def sylsp_bytes(kmers, counts, c=200, k=31, file_name=b"reads.fq", sample_name=None, paired=True, mean=151.5, n_field=None):
    tail = struct.pack("<QQ", c, k) + struct.pack("<Q", len(file_name)) + file_name
    tail += (b"\x01" + struct.pack("<Q", len(sample_name)) + sample_name) if sample_name is not None else b"\x00"
    tail += struct.pack("<B", int(paired)) + struct.pack("<d", mean)
    return struct.pack("<Q", len(kmers) if n_field is None else n_field) + pack_entries(kmers, counts).tobytes() + tail


@pytest.fixture(scope="module")
def host():
    H = C.CDLL(os.path.join(ROOT, "sylph_amd", "libsylph_host.so"))
    H.sylph_host_read_sylsp.argtypes = [C.c_char_p, vp, vp, u64] + [vp] * 5 + [C.c_char_p, C.c_char_p, u64, vp]
    H.sylph_host_read_sylsp_header.argtypes = [C.c_char_p] + [vp] * 6 + [C.c_char_p, C.c_char_p, u64, vp, C.c_char_p, u64]
    H.sylph_host_sylsp_error.argtypes = [C.c_char_p, C.c_char_p, u64]
    return H


def read_both(H, path):
    """-> (metadata by read_sylsp, metadata + entry count + offset by read_sylsp_header), or the two error messages"""
    n, c, k, pr, hs = u64(), u64(), u64(), C.c_int(), C.c_int()
    mean = C.c_double()
    fn, sn = C.create_string_buffer(512), C.create_string_buffer(512)
    rc_a = H.sylph_host_read_sylsp(path, None, None, 0, C.byref(n), C.byref(c), C.byref(k), C.byref(pr), C.byref(mean), fn, sn, 512, C.byref(hs))
    a = (c.value, k.value, pr.value, mean.value, fn.value, sn.value, hs.value)
    n_table = n.value
    ne, off, err = u64(), u64(), C.create_string_buffer(1024)
    rc_b = H.sylph_host_read_sylsp_header(path, C.byref(ne), C.byref(off), C.byref(c), C.byref(k), C.byref(pr), C.byref(mean), fn, sn, 512,
                                          C.byref(hs), err, 1024)
    b = (c.value, k.value, pr.value, mean.value, fn.value, sn.value, hs.value)
    err_a = C.create_string_buffer(1024)
    assert (H.sylph_host_sylsp_error(path, err_a, 1024) == 0) == (rc_a == 0)
    return rc_a, rc_b, a, b, n_table, ne.value, off.value, err_a.value, err.value


def test_header_reader_agrees_with_read_sylsp(host, tmp_path):
    kmers, counts = entries_case("duplicates", 2 * T + 1, seed=1)
    for i, (sample, paired, trailing) in enumerate([(None, True, b""), (b"gut sample", False, b""), (b"", True, b"trailing bytes are tolerated")]):
        p = tmp_path / f"s{i}.sylsp"
        p.write_bytes(sylsp_bytes(kmers, counts, sample_name=sample, paired=paired, mean=100.25 + i) + trailing)
        rc_a, rc_b, a, b, n_table, n_entries, off, _, _ = read_both(host, str(p).encode())
        assert rc_a == 0 and rc_b == 0 and a == b
        assert a == (200, 31, int(paired), 100.25 + i, b"reads.fq", sample or b"", int(sample is not None))
        assert n_entries == len(kmers) and n_table == len(model_table(kmers, counts)[0]) < n_entries
        assert p.read_bytes()[off:off + 12 * n_entries] == pack_entries(kmers, counts).tobytes() and off == 8   # where the view says the entries lie
    p = tmp_path / "empty.sylsp"
    p.write_bytes(sylsp_bytes(kmers[:0], counts[:0]))
    rc_a, rc_b, a, b, n_table, n_entries, _, _, _ = read_both(host, str(p).encode())
    assert rc_a == 0 and rc_b == 0 and a == b and n_table == n_entries == 0


def test_header_reader_fails_as_read_sylsp_does(host, tmp_path):
    kmers, counts = entries_case("ascending", 100, seed=0)
    good = sylsp_bytes(kmers, counts, sample_name=b"x")
    table_end = 8 + 12 * 100
    cases = {"truncated_table": good[:8 + 12 * 57 + 5], "table_ends_the_file": good[:table_end],
             "n_times_12_wraps": sylsp_bytes(kmers, counts, n_field=2**64 // 12 + 3), "n_times_12_huge": sylsp_bytes(kmers, counts, n_field=2**61),
             "truncated_tail_in_c": good[:table_end + 4], "truncated_tail_in_name": good[:table_end + 16 + 8 + 3],
             "truncated_tail_in_mean": good[:-1], "empty_file": b"", "only_the_length": good[:8]}
    for name, blob in cases.items():
        p = tmp_path / f"{name}.sylsp"
        p.write_bytes(blob)
        rc_a, rc_b, _, _, _, _, _, err_a, err_b = read_both(host, str(p).encode())
        assert rc_a == -1 and rc_b == -1, name
        assert err_a == err_b and b"is not a valid sketch" in err_a and str(p).encode() in err_a, (name, err_a, err_b)
    rc_a, rc_b, *_, err_a, err_b = read_both(host, str(tmp_path / "missing.sylsp").encode())
    assert rc_a == -1 and rc_b == -1 and err_a == err_b and b"could not be opened" in err_a


def test_standalone_program_runs_clean_under_the_sanitizers():
    """tests/sylsp_plan_sanitize_main.cpp + the model, built with AddressSanitizer and UBSan into a program of its own and run on
    the CPU: nothing is loaded into this interpreter."""
    srcs = [os.path.join(HERE, "sylsp_plan_sanitize_main.cpp"), SRC]
    exe, stale = build_path("sylph_sylsp_plan_sanitize", srcs + [HDR])
    if stale:
        tmp = exe + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                               "-Werror", "-o", tmp] + srcs)
        os.replace(tmp, exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "sylsp plan sanitize run ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    assert " 0 cases" not in p.stdout and " 0 sorted" not in p.stdout and " 0 ascending" not in p.stdout
