"""CPU tests of the hit finish's plan (sylph_amd/csrc/hits_plan.h, the very header hits.hip's kernels and contain.hip's finish_driver
include, compiled with g++ through tests/hits_plan_capi.cpp): the stretches of the hit list, the row counters' bijection, the geometry of
an assembly against a restatement of the formulas, the two row lists, the verdict's table, the capacity rules — and every walk of the
driver's state function from every start under every sequence of answers, with the clean/dirty record checked against a model of what
the kernels zero.  Plus the stand-alone sanitizer run."""
import ctypes as C
import os
import subprocess
from collections import namedtuple

import numpy as np
import pytest

from . import contain_edges as E
from .helpers import build_path

HERE = os.path.dirname(os.path.abspath(__file__))
HDR = os.path.join(HERE, "..", "sylph_amd", "csrc", "hits_plan.h")
SRC = os.path.join(HERE, "hits_plan_capi.cpp")

REGROW, SORTED, ROWS = range(3)                                                  # Verdict
DEVICE, HOST = range(2)                                                          # Sizes
PROBE, ASSEMBLE, READ, REGROW_PROBE, SORT, COPY_OUT, DONE, FAIL = range(8)       # Step
ENDS = (SORT, COPY_OUT, DONE, FAIL)
St = namedtuple("St", "to_probe sizes force_sort rows_taken finish probes assembled read verdict rc_dirty cnt_dirty")
WIDTHS = (1, 1, 1, 1, 1, 2, 1, 1, 2, 1, 1)
TOP = 2**32 - 1


def unword(w):
    out = []
    for bits in WIDTHS:
        out.append(w & ((1 << bits) - 1))
        w >>= bits
    return St(*out)


@pytest.fixture(scope="module")
def L():
    out, stale = build_path("sylph_hits_plan", [SRC, HDR], ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, SRC])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    u32, u64, ptr = C.c_uint32, C.c_uint64, C.c_void_p
    for name, res, args in (("hp_constants", None, [ptr]), ("hp_hash_row", u32, [u32]), ("hp_rc_at", u32, [u32, u32]),
                            ("hp_stretch_of", None, [u32, u32, u32, ptr, ptr]), ("hp_stretch_check", u32, [u32, u32]),
                            ("hp_rc_bijection", C.c_int, [u32]), ("hp_rc_shared_lines", u64, [u32, u32, u32]),
                            ("hp_geometry", None, [u64, u64, u64, ptr]), ("hp_first_capacity", u64, [u64]), ("hp_fits", C.c_int, [u64]),
                            ("hp_verdict", C.c_int, [u32, u32, u32]), ("hp_place_rows", u64, [ptr, u64, u64, ptr]),
                            ("hp_start", u32, [C.c_int] * 8), ("hp_next", C.c_int, [u32]), ("hp_after", u32, [u32, C.c_int, C.c_int]),
                            ("hp_failed", u32, [u32]), ("hp_behind_probe", C.c_int, [u32]), ("hp_walk_all", None, [ptr])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    k = (u32 * 9)()
    lib.hp_constants(k)
    lib.K = dict(zip("ROWS_TPB ROWS_PER_THREAD ROWS_TILE SMALL_ROW MAX_VALUE_LDS HIT_SLOTS HIT_SLOTS_FULL STRETCH_ROUND MAX_PROBES".split(), k))
    return lib


def test_constants_are_the_ones_the_edge_inputs_are_written_around(L):
    K = L.K
    assert (K["ROWS_TILE"], K["SMALL_ROW"], K["MAX_VALUE_LDS"]) == (E.ROWS_TILE, E.SMALL_ROW, E.MAX_VALUE_LDS) == (2048, 64, 4096)
    assert K["ROWS_TPB"] * K["ROWS_PER_THREAD"] == K["ROWS_TILE"] and K["STRETCH_ROUND"] == 256 and K["MAX_PROBES"] == 2
    assert K["HIT_SLOTS_FULL"] == K["HIT_SLOTS"] * 3 // 4 and K["HIT_SLOTS_FULL"] + K["STRETCH_ROUND"] <= K["HIT_SLOTS"]
    assert K["HIT_SLOTS"] & (K["HIT_SLOTS"] - 1) == 0
    rows = np.random.default_rng(1).integers(0, 2**32, size=4096, dtype=np.uint64)
    assert all(L.hp_hash_row(int(r)) == ((int(r) * 2654435761) % 2**32) >> (32 - K["HIT_SLOTS"].bit_length() + 1) < K["HIT_SLOTS"] for r in rows)


# ------------------------------------------------------------------------------------------------------------------- stretches
STRETCH_N = (0, 1, 255, 256, 257, 6143, 6144, 2**20 + 1, TOP)
STRETCH_GRIDS = (16, 17, 64, 768)


@pytest.mark.parametrize("grid", STRETCH_GRIDS)
def test_stretches_are_disjoint_and_cover_the_list_in_block_order(L, grid):
    lo, hi = C.c_uint32(), C.c_uint32()
    for n in STRETCH_N:
        assert L.hp_stretch_check(n, grid) == 0, (n, grid)
        # the same in exact integers: nothing wrapped at the top of uint32_t
        per = (-(-n // grid) + 255) // 256 * 256                    # the hits per workgroup, rounded up to whole rounds
        assert (grid - 1) * per < 2**32
        at = 0
        for b in range(grid):
            L.hp_stretch_of(n, grid, b, C.byref(lo), C.byref(hi))
            assert (lo.value, hi.value) == (min(n, b * per), min(n, b * per + per)), (n, grid, b)
            assert lo.value == at and (lo.value % 256 == 0 or lo.value == n)
            at = hi.value
        assert at == n


def test_stretches_at_random_sizes_near_the_top(L):
    rng = np.random.default_rng(7)
    sizes = np.concatenate([rng.integers(0, 2**32, size=200, dtype=np.uint64), TOP - rng.integers(0, 2000, size=200, dtype=np.uint64)])
    for n in sizes.tolist():
        grid = max(16, min(n // 6144, 768))                         # what geometry() hands out for n hits
        assert L.hp_stretch_check(n, grid) == 0, (n, grid)
        assert L.hp_stretch_check(n, max(16, min(n // 2 // 6144, 768))) == 0     # ... and for a device-sized list that filled its array


def test_the_former_expression_wrapped_at_the_top(L):
    """What stretch_of replaced, ((n + grid - 1) / grid + 255) & ~255 and hi = min(n, lo + per) in uint32_t: for 2^32 - 1 hits the sum
    n + grid - 1 wraps and no workgroup of 768 (or of 16) takes a hit; for 2^32 - 16 hits and 16 workgroups lo + per wraps and the last stretch is empty.  Up to
    2^32 - 1 - 256 * 768 hits nothing can wrap (grid * per < n + 256 * grid) and the two spellings agree."""
    M = 2**32

    def former(n, grid, b):
        per = ((n + grid - 1) % M // grid + 255) % M & ~255 & (M - 1)
        lo = min(n, b * per % M)
        return lo, min(n, (lo + per) % M)
    assert all(former(TOP, 768, b) == (0, 0) for b in range(768))
    assert all(former(TOP, 16, b) == (0, 0) for b in range(16))
    assert former(M - 16, 16, 14) == (14 * 2**28, 15 * 2**28) and former(M - 16, 16, 15) == (15 * 2**28, 0)
    assert L.hp_stretch_check(M - 16, 16) == 0
    lo, hi = C.c_uint32(), C.c_uint32()
    for n in STRETCH_N[:-1] + (TOP - 256 * 768,):
        for grid in STRETCH_GRIDS:
            for b in (0, 1, grid // 2, grid - 1):
                L.hp_stretch_of(n, grid, b, C.byref(lo), C.byref(hi))
                assert (lo.value, hi.value) == former(n, grid, b), (n, grid, b)


# ------------------------------------------------------------------------------------------------------------------- row counters
MULT = 0x9E3779B1


def test_rc_at_is_a_bijection_that_spreads_neighbours_over_lines(L):
    assert MULT % 2 == 1                                             # odd: invertible modulo every power of two
    for m in range(10, 23):
        R2 = 1 << m
        assert L.hp_rc_bijection(R2) == 1, R2
        assert L.hp_rc_shared_lines(R2, 0, R2 - 16) == 0, R2        # 16 consecutive rows: 16 different 64-byte lines of 16 counters
    rng = np.random.default_rng(3)
    for m in range(23, 32):                                          # (geometry() never goes beyond 2^31 counters)
        R2, inv = 1 << m, pow(MULT, -1, 1 << m)
        rows = rng.integers(0, R2, size=500, dtype=np.uint64).tolist() + [0, 1, R2 - 1]
        for r in rows:
            a = L.hp_rc_at(r, R2 - 1)
            assert a == r * MULT % R2 and a * inv % R2 == r
        for r in rows[:50]:
            assert L.hp_rc_shared_lines(R2, min(r, R2 - 16), 1) == 0


# ------------------------------------------------------------------------------------------------------------------- geometry
GEOMETRY_ROWS = sorted(set(E.TINY_G + [3 * g for g in E.TINY_G] + [E.MANY_TILES_S * E.MANY_TILES_G, 2**31 - 1]))
GEOMETRY_CAPS = (1, 2**20, TOP)
G = namedtuple("G", "taken R R2 rc_mask n_tiles list_cap hit_grid rc_bytes meta_bytes tile_sum_at snap_at lists_at")


def geometry(L, n_rows, cap, n_guess):
    out = (C.c_uint64 * 12)()
    L.hp_geometry(n_rows, cap, n_guess, out)
    return G(*[int(x) for x in out])


def test_geometry_equals_the_formulas_and_its_regions_are_disjoint(L):
    assert 524_352 in GEOMETRY_ROWS
    for n_rows in GEOMETRY_ROWS:
        for cap in GEOMETRY_CAPS:
            for n_guess in (cap // 2, cap, 0, 16 * 6144 - 1, 16 * 6144 + 6144, 768 * 6144, 769 * 6144):
                g = geometry(L, n_rows, cap, n_guess)
                R2 = 1024
                while R2 < n_rows:
                    R2 <<= 1
                n_tiles, list_cap = -(-n_rows // 2048), min(n_rows, max(cap, 1))
                want = G(1, n_rows, R2, R2 - 1, n_tiles, list_cap, max(16, min(n_guess // 6144, 768)), R2 * 4, (n_tiles + 4 + 2 + list_cap) * 4 + 64,
                         0, n_tiles, n_tiles + 4)
                assert g == want, (n_rows, cap, n_guess)
                assert g.R2 >= g.R and g.R2 & (g.R2 - 1) == 0 and 16 <= g.hit_grid <= 768
                assert g.rc_bytes >= 4 * (max(L.hp_rc_at(r, g.rc_mask) for r in (0, 1, g.R // 2, g.R - 1)) + 1)
                # [tile_sum | snap | lists: two lengths, list_cap rows] side by side, all inside meta_bytes
                regions = [(g.tile_sum_at, g.n_tiles), (g.snap_at, 4), (g.lists_at, 2 + g.list_cap)]
                assert all(a + n <= b for (a, n), (b, _) in zip(regions, regions[1:]))
                assert (g.lists_at + 2 + g.list_cap) * 4 <= g.meta_bytes
    for n_rows in (0, 2**31, 2**31 + 1, 2**32 - 2):
        for cap in GEOMETRY_CAPS:
            assert geometry(L, n_rows, cap, cap) == G(*[0] * 12)


# ------------------------------------------------------------------------------------------------------------------- the two row lists
def row_count_vectors():
    rng = np.random.default_rng(11)
    R = 5000
    yield "all small", np.full(R, 64, dtype=np.uint32)
    yield "all long", np.full(R, 65, dtype=np.uint32)
    yield "alternating", np.where(np.arange(R) % 2 == 0, 1, 65).astype(np.uint32)
    one = np.zeros(R, dtype=np.uint32)
    one[R // 2] = 3_000_000
    yield "one row holds everything", one
    yield "every row one hit", np.ones(R, dtype=np.uint32)
    yield "a single row", np.array([1], dtype=np.uint32)
    yield "a single long row", np.array([65], dtype=np.uint32)
    for i in range(20):
        c = rng.choice([0, 0, 1, 2, 63, 64, 65, 66, 1000], size=int(rng.integers(1, R))).astype(np.uint32)
        yield f"random {i}", c


def test_row_lists_never_meet_and_never_leave_their_region(L):
    out = (C.c_uint32 * 2)()
    for name, counts in row_count_vectors():
        total = int(counts.sum())
        for cap in sorted({max(total, 1), total + 1, 2 * total + 7, 2**20}):          # the sum is at most cap; the tightest array first
            if cap < total:
                continue
            assert L.hp_place_rows(counts.ctypes.data, len(counts), cap, out) == 0, (name, cap)
            assert out[0] == int(((counts > 0) & (counts <= 64)).sum()) and out[1] == int((counts > 64).sum()), name
            assert out[0] + out[1] <= min(len(counts), max(cap, 1))
    # the model does notice a list that is too short: more listed rows than the array has entries
    counts = np.ones(100, dtype=np.uint32)
    assert L.hp_place_rows(counts.ctypes.data, len(counts), 50, out) == 51
    mixed = np.where(np.arange(100) % 2 == 0, 1, 65).astype(np.uint32)
    assert L.hp_place_rows(mixed.ctypes.data, len(mixed), 60, out) != 0


# ------------------------------------------------------------------------------------------------------------------- verdict, capacity
def test_verdict_table(L):
    """As the code behaved before there was a plan: rows_sum_kernel's snap[2] = largest value >= 4096 or the probe overflowed, the host's
    n_hits > cap first (once more with a larger array), then the value.  Overflow wins: a probe that overflowed did not see every count."""
    table = {  # (n_counted relative to cap, max_count) -> verdict
        ("0", 0): ROWS, ("0", 4095): ROWS, ("0", 4096): SORTED, ("0", TOP): SORTED,
        ("cap-1", 0): ROWS, ("cap-1", 4095): ROWS, ("cap-1", 4096): SORTED, ("cap-1", TOP): SORTED,
        ("cap", 0): ROWS, ("cap", 4095): ROWS, ("cap", 4096): SORTED, ("cap", TOP): SORTED,
        ("cap+1", 0): REGROW, ("cap+1", 4095): REGROW, ("cap+1", 4096): REGROW, ("cap+1", TOP): REGROW,
    }
    for cap in (1, 2, 4096, 2**20, TOP - 1, TOP):
        for (rel, mx), want in table.items():
            n = {"0": 0, "cap-1": cap - 1, "cap": cap, "cap+1": cap + 1}[rel]
            if n > TOP:
                continue                                            # (a device word cannot say so)
            assert L.hp_verdict(n, mx, cap) == want, (cap, rel, mx)


def test_first_capacity_and_the_limit(L):
    totals = [0, 1, 2**19 - 1, 2**19, 2**19 + 1, 2**20, 10**7, 2**31 - 1, 2**31, TOP]
    caps = [L.hp_first_capacity(t) for t in totals]
    assert caps == [max(2 * t, 1 << 20) for t in totals]
    assert all(a <= b for a, b in zip(caps, caps[1:])) and min(caps) == 2**20
    assert [L.hp_fits(c) for c in (0, 1, 2**20, TOP, 2**32, 2**32 + 1, 2**33)] == [1, 1, 1, 1, 0, 0, 0]
    assert L.hp_fits(L.hp_first_capacity(2**31 - 1)) and not L.hp_fits(L.hp_first_capacity(2**31))


# ------------------------------------------------------------------------------------------------------------------- the state function
def starts(L):
    for bits in range(128):
        for known in (SORTED, ROWS):
            to_probe = bits & 1
            if to_probe and known != ROWS:
                continue
            yield L.hp_start(to_probe, bits >> 1 & 1, bits >> 2 & 1, bits >> 3 & 1, bits >> 4 & 1, bits >> 5 & 1, bits >> 6 & 1, known)


def walks(L, w0):
    """every walk from w0: (steps, answers given to ReadWords, the state in front of the last step)"""
    out = []

    def go(w, steps, answers):
        assert len(steps) <= 16, ("a walk that does not end", steps)
        step = L.hp_next(w)
        if step in ENDS:
            out.append((steps + [step], answers, unword(w)))
            return
        for a in ((REGROW, SORTED, ROWS) if step == READ else (ROWS,)):
            go(L.hp_after(w, step, a), steps + [step], answers + ([a] if step == READ else []))
    go(w0, [], [])
    return out


def test_every_walk_ends_probes_twice_at_most_and_fails_exactly_on_a_second_overflow(L):
    n_walks, n_failed, ends, longest = 0, 0, set(), 0
    for w0 in starts(L):
        s0 = unword(w0)
        for steps, answers, s in walks(L, w0):
            n_walks += 1
            ends.add(steps[-1])
            longest = max(longest, len(steps))
            probes, assemblies = steps.count(PROBE) + steps.count(REGROW_PROBE), steps.count(ASSEMBLE)
            assert probes <= 2 and assemblies <= 2 and steps.count(PROBE) == s0.to_probe and all(x not in ENDS for x in steps[:-1]), steps
            assert (steps[-1] == FAIL) == (answers == [REGROW, REGROW]), (steps, answers)
            n_failed += steps[-1] == FAIL
            assert steps.count(READ) == probes                       # every probe's words are read, once
            row_road = not s0.force_sort and s0.rows_taken
            if not row_road:
                assert assemblies == 0 and steps[-1] != COPY_OUT
            if not s0.finish:
                assert steps[-1] in (DONE, FAIL) and assemblies == (probes if row_road and s0.sizes == DEVICE else 0)
            elif steps[-1] != FAIL:
                final = answers[-1] if answers else s0.verdict
                assert steps[-1] == (COPY_OUT if row_road and final == ROWS else SORT), (steps, answers)
                assert steps[-1] != COPY_OUT or steps[-2] in (ASSEMBLE, READ)
            # the assembly runs behind the probe, in front of the words, on the device-sized row road only
            for i, x in enumerate(steps):
                if x in (PROBE, REGROW_PROBE):
                    assert steps[i + 1] == (ASSEMBLE if row_road and s0.sizes == DEVICE else READ), steps
    out = (C.c_uint64 * 14)()
    L.hp_walk_all(out)                                               # the C++ walk, with the model of the device's memory beside it
    assert out[0] == n_walks and out[1] == 0 and out[2] == n_failed > 0 and out[3] == longest and out[4] == 2 and out[5] == 2
    assert ends == set(ENDS) and [out[6 + e] > 0 for e in range(8)] == [e in ENDS for e in range(8)]


def road(L, answers, to_probe=1, sizes=DEVICE, force_sort=0, rows_taken=1, finish=1, rc_dirty=0, cnt_dirty=0, known=ROWS):
    """one walk -> (its steps, rc_dirty and cnt_dirty behind it)"""
    w = L.hp_start(to_probe, sizes, force_sort, rows_taken, finish, rc_dirty, cnt_dirty, known)
    answers, steps = list(answers), []
    while True:
        step = L.hp_next(w)
        steps.append(step)
        if step in ENDS:
            assert not answers
            return steps, unword(w).rc_dirty, unword(w).cnt_dirty
        w = L.hp_after(w, step, answers.pop(0) if step == READ else ROWS)


def test_roads_and_their_record(L):
    """the launches of every road as they were before there was a plan, and what each leaves clean (0) or dirty (1)"""
    # a sample or a batch against the database: the assembly behind the probe; rows_sort_kernel zeroes the two words, the row sort the counters
    assert road(L, [ROWS]) == ([PROBE, ASSEMBLE, READ, COPY_OUT], 0, 0)
    assert road(L, [ROWS], rc_dirty=1, cnt_dirty=1) == ([PROBE, ASSEMBLE, READ, COPY_OUT], 0, 0)
    # a value of 4096: the assembly stopped behind snap[2]; the sorted finish from the same list; nothing was zeroed
    assert road(L, [SORTED]) == ([PROBE, ASSEMBLE, READ, SORT], 1, 1)
    # the hit list outgrew its array: probe and assembly once more
    assert road(L, [REGROW, ROWS]) == ([PROBE, ASSEMBLE, READ, REGROW_PROBE, ASSEMBLE, READ, COPY_OUT], 0, 0)
    assert road(L, [REGROW, SORTED]) == ([PROBE, ASSEMBLE, READ, REGROW_PROBE, ASSEMBLE, READ, SORT], 1, 1)
    assert road(L, [REGROW, REGROW]) == ([PROBE, ASSEMBLE, READ, REGROW_PROBE, ASSEMBLE, READ, FAIL], 1, 1)
    # SYLPH_HIP_HIT_SORT, no rows, rows beyond the assembly: the host waits for the words and sorts; the counters are not touched
    for kw in (dict(force_sort=1), dict(rows_taken=0)):
        assert road(L, [ROWS], **kw) == ([PROBE, READ, SORT], 0, 1)
        assert road(L, [ROWS], rc_dirty=1, **kw) == ([PROBE, READ, SORT], 1, 1)
        assert road(L, [REGROW, ROWS], **kw) == ([PROBE, READ, REGROW_PROBE, READ, SORT], 0, 1)
        assert road(L, [], to_probe=0, **kw) == ([SORT], 0, 0)
    # nothing to probe (an empty table, an empty index): an all-zero block through the same kernels, host-known sizes
    assert road(L, [], to_probe=0) == ([ASSEMBLE, COPY_OUT], 0, 0)
    assert road(L, [], to_probe=0, rc_dirty=1, cnt_dirty=1) == ([ASSEMBLE, COPY_OUT], 0, 1)
    # the reassignment pass: its launch counts into the two words, the host waits, the assembly takes host-known sizes and leaves the words
    assert road(L, [ROWS], sizes=HOST) == ([PROBE, READ, ASSEMBLE, COPY_OUT], 0, 1)
    assert road(L, [SORTED], sizes=HOST) == ([PROBE, READ, SORT], 0, 1)
    assert road(L, [REGROW, ROWS], sizes=HOST) == ([PROBE, READ, REGROW_PROBE, READ, ASSEMBLE, COPY_OUT], 0, 1)
    assert road(L, [REGROW, REGROW], sizes=HOST) == ([PROBE, READ, REGROW_PROBE, READ, FAIL], 0, 1)
    # the sharded exchange: the probe for the hit list alone, later the finish with host-known sizes
    assert road(L, [ROWS], sizes=HOST, finish=0) == ([PROBE, READ, DONE], 0, 1)
    assert road(L, [SORTED], sizes=HOST, finish=0) == ([PROBE, READ, DONE], 0, 1)
    assert road(L, [REGROW, SORTED], sizes=HOST, finish=0) == ([PROBE, READ, REGROW_PROBE, READ, DONE], 0, 1)
    assert road(L, [], to_probe=0, sizes=HOST, finish=0) == ([DONE], 0, 0)
    assert road(L, [], to_probe=0, sizes=HOST, cnt_dirty=1) == ([ASSEMBLE, COPY_OUT], 0, 1)
    assert road(L, [], to_probe=0, sizes=HOST, known=SORTED, rc_dirty=1) == ([SORT], 1, 0)
    # a step that threw half-way: nothing is known to be clean
    w = L.hp_failed(L.hp_start(1, DEVICE, 0, 1, 1, 0, 0, ROWS))
    assert (unword(w).rc_dirty, unword(w).cnt_dirty) == (1, 1)


def test_standalone_program_runs_clean_under_the_sanitizers():
    """tests/hits_plan_sanitize_main.cpp + the wrapper, built with AddressSanitizer and UBSan into a program of its own and run on the
    CPU: nothing is loaded into this interpreter."""
    srcs = [os.path.join(HERE, "hits_plan_sanitize_main.cpp"), SRC]
    exe, stale = build_path("sylph_hits_plan_sanitize", srcs + [HDR])
    if stale:
        tmp = exe + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                               "-Werror", "-o", tmp] + srcs)
        os.replace(tmp, exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "hits plan sanitize run ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    assert " 0 walks" not in p.stdout and "at most 2 probes and 2 assemblies" in p.stdout
