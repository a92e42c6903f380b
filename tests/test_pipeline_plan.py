"""CPU tests of the sample pipeline's scheduler.  sylph_amd/csrc/pipeline_plan.h (what the pipeline decides; compiled with g++ through
tests/pipeline_plan_capi.cpp): the probe-batch rule over every small case against a restatement, that a sharded batch's size is a
function of the flush points alone and its start of its own samples alone, that sylph_pipeline_next refuses exactly when no worker's
progress could wake it, the slots of a result block, the router's choice with both refusals, and the defaults against the numbers
include/sylph_hip.h quotes.  sylph_amd/csrc/pipeline_core.h (the threads and queues): tests/pipeline_core_main.cpp, a program of its
own over a fake work interface, under ThreadSanitizer and under AddressSanitizer + UBSan."""
import ctypes as C
import itertools
import os
import re
import subprocess

import pytest

from .helpers import build_path

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "sylph_amd", "csrc")
PLAN, CORE = os.path.join(CSRC, "pipeline_plan.h"), os.path.join(CSRC, "pipeline_core.h")
SRC = os.path.join(HERE, "pipeline_plan_capi.cpp")
CORE_MAIN = os.path.join(HERE, "pipeline_core_main.cpp")

QUEUED, SKETCHING, SKETCHED = range(3)       # JobState (Profiled cannot follow the first sample that is not profiled)
MAX_LEN = 6
# every set of at most three flush points out of first + 0 .. first + 6, as bit masks
MASKS = [sum(1 << b for b in pts) for k in range(4) for pts in itertools.combinations(range(MAX_LEN + 1), k)]


@pytest.fixture(scope="module")
def L():
    out, stale = build_path("sylph_pipeline_plan", [SRC, PLAN], ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, SRC])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    lib.pp_batch_table.argtypes = [C.c_uint32, C.c_int, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.pp_wait_for_fuller.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64]
    lib.pp_next_would_block.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32]
    lib.pp_flush_point_spent.argtypes = [C.c_uint64, C.c_uint64]
    lib.pp_slots.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
    lib.pp_pick_replica.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
    lib.pp_defaults.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.pp_router_depth.argtypes = [C.c_uint32, C.c_uint32]
    lib.pp_router_depth.restype = C.c_uint32
    lib.pp_sharded_depth_ok.argtypes = [C.c_uint32, C.c_uint32]
    return lib


def batch_rule(states, max_batch, sharded, first, flush):
    """The rule restated -> (samples in the batch, whether it goes now)."""
    want = max_batch
    beyond = [f for f in sorted(flush) if f > first]
    if sharded and beyond:
        want = min(want, beyond[0] - first)
    run = 0
    while run < min(want, len(states)) and states[run] == SKETCHED:
        run += 1
    return (want, run == want) if sharded else (run, run > 0)


def batch_table(L, max_batch, sharded, length, first=0):
    """{(states, mask): (n, go)} of the header, for every state vector of that length and every set of flush points"""
    masks = (C.c_uint32 * len(MASKS))(*MASKS)
    out = (C.c_uint16 * (3 ** length * len(MASKS)))()
    L.pp_batch_table(max_batch, sharded, length, first, masks, len(MASKS), out)
    vectors = [tuple(v // 3 ** i % 3 for i in range(length)) for v in range(3 ** length)]
    return {(st, m): (out[i * len(MASKS) + k] & 255, bool(out[i * len(MASKS) + k] >> 8)) for i, st in enumerate(vectors) for k, m in enumerate(MASKS)}


def points(mask, first=0):
    return [first + b for b in range(32) if mask >> b & 1]


@pytest.mark.parametrize("max_batch", [1, 2, 3, 4])
def test_batch_rule_over_every_small_case(L, max_batch):
    n_go = 0
    for sharded in (0, 1):
        for length in range(MAX_LEN + 1):
            table = batch_table(L, max_batch, sharded, length)
            assert len(table) == 3 ** length * len(MASKS) == 3 ** length * 64
            for (st, m), got in table.items():
                assert got == batch_rule(st, max_batch, sharded, 0, points(m)), (sharded, st, points(m), got)
                n, go = got
                n_go += go
                if go:          # a batch that goes is sketched samples only, at most max_batch, and never reaches across a flush point
                    assert 1 <= n <= min(max_batch, length) and all(s == SKETCHED for s in st[:n])
                    assert not sharded or not any(0 < f < n for f in points(m)), (st, points(m), n)
                if not sharded:  # every ready sample up to max_batch goes at once; flush points mean nothing
                    assert go == (length > 0 and st[0] == SKETCHED) and got == table[(st, 0)]
                    assert n == max_batch or n == length or st[n] != SKETCHED
            if sharded:
                # the size is a function of the call sequence (max_batch, the flush points) alone, and whether the batch goes depends
                # on its own samples alone: never on which samples beyond it are sketched
                for m in MASKS:
                    sizes = {table[(st, m)][0] for st in itertools.product(range(3), repeat=length)}
                    assert len(sizes) == 1
                    n = sizes.pop()
                    assert n == min([max_batch] + [f for f in points(m) if f > 0][:1])
                    for st in itertools.product(range(3), repeat=length):
                        assert table[(st, m)][1] == (length >= n and all(s == SKETCHED for s in st[:n]))
    assert n_go > 0
    # sequence numbers only count from the first sample that is not profiled
    for sharded in (0, 1):
        assert list(batch_table(L, max_batch, sharded, 4, first=10 ** 12).values()) == list(batch_table(L, max_batch, sharded, 4).values())


def test_spent_flush_points_and_the_wait_for_a_fuller_batch(L):
    assert [L.pp_flush_point_spent(p, 5) for p in (0, 4, 5, 6)] == [1, 1, 1, 0]
    for batch, min_batch, max_batch, wait_us, sharded, coming in itertools.product(range(5), range(5), range(1, 5), (0, 400), (0, 1), range(3)):
        want = not sharded and wait_us > 0 and batch < min(min_batch, max_batch) and coming > 0
        assert L.pp_wait_for_fuller(batch, min_batch, max_batch, wait_us, sharded, coming) == want
    d = (C.c_uint32 * 5)()
    L.pp_defaults(0, 0, 0, d)
    assert not any(L.pp_wait_for_fuller(b, d[3], d[2], d[4], 0, 3) for b in range(1, 9))      # min_batch 1: a ready table never waits


@pytest.mark.parametrize("max_batch", [1, 2, 3, 4])
def test_next_refuses_exactly_when_no_worker_could_wake_it(L, max_batch):
    """With every outstanding sample set to Sketched — all that the workers alone can bring about — the front sample's batch goes or it
    never will: sylph_pipeline_next must refuse (SYLPH_ERR_STATE) in exactly the second case.  A flush point is a number of submitted
    samples, so it lies at or below first + outstanding."""
    refused = 0
    for length in range(1, MAX_LEN + 1):
        table = batch_table(L, max_batch, 1, length)
        for m in MASKS:
            if any(f > length for f in points(m)):
                continue
            goes = table[((SKETCHED,) * length, m)][1]
            blocks = L.pp_next_would_block(1, 0, any(f > 0 for f in points(m)), length, max_batch)
            assert blocks == (not goes), (length, points(m))
            refused += blocks
            assert not L.pp_next_would_block(0, 0, any(f > 0 for f in points(m)), length, max_batch)       # unsharded: one sketched sample goes
            assert not L.pp_next_would_block(1, 1, 0, length - 1, max_batch)                                # the front sample is done already
    assert refused == 2 * (max_batch - 1)       # per number of samples below max_batch: the sets without a point beyond the front, {} and {first}


def test_slots_in_a_shared_result_block(L):
    for n in range(MAX_LEN + 1):
        for good in itertools.product((0, 1), repeat=n):
            out = (C.c_int32 * max(n, 1))()
            L.pp_slots(bytes(good), n, 1, out)
            assert [out[i] for i in range(n)] == [sum(good[:i]) if g else -1 for i, g in enumerate(good)]      # consecutive, in batch order
            L.pp_slots(bytes(good), n, 0, out)
            assert [out[i] for i in range(n)] == [-1] * n                                                    # a failed probe fails them all


def test_the_routers_choice_and_its_two_refusals(L):
    none_there, all_full = L.pp_no_replica_on_device(), L.pp_all_full()
    assert none_there < 0 and all_full < 0 and none_there != all_full
    seen = set()
    for n in range(1, 4):
        for reps in itertools.product(itertools.product((0, 1), range(3), (1, 2)), repeat=n):       # (device, outstanding, depth) per replica
            dev = (C.c_int32 * n)(*[r[0] for r in reps])
            out = (C.c_uint32 * n)(*[r[1] for r in reps])
            depth = (C.c_uint32 * n)(*[r[2] for r in reps])
            for want in (-1, 0, 1, 2):
                there = [i for i, r in enumerate(reps) if want < 0 or r[0] == want]
                free = [i for i in there if reps[i][1] < reps[i][2]]
                # the fewest outstanding below its depth; among equals the first
                expect = min(free, key=lambda i: (reps[i][1], i)) if free else all_full if there else none_there
                got = L.pp_pick_replica(dev, out, depth, n, want)
                assert got == expect, (reps, want, got)
                seen.add("ok" if got >= 0 else got)
    assert seen == {"ok", none_there, all_full}


def test_defaults_are_the_numbers_the_public_header_quotes(L):
    with open(os.path.join(HERE, "..", "include", "sylph_hip.h")) as f:
        header = f.read()
    assert "pipeline_plan.h" in header
    workers = int(re.search(r"uint32_t n_workers;\s*/\* [^*]*0 = default \((\d+)\)", header).group(1))
    beyond = int(re.search(r"uint32_t depth;\s*/\* [^*]*0 = n_workers \+ (\d+) \*/", header).group(1))
    max_batch = int(re.search(r"uint32_t max_batch;\s*/\* [^*]*0 = default \((\d+)\)", header).group(1))
    min_batch, wait_us = map(int, re.search(r'"min_batch" \+\s*\*?\s*"batch_wait_us" \(default (\d+) / (\d+)', header).groups())
    assert (workers, beyond, max_batch, min_batch, wait_us) == (3, 5, 8, 1, 400)
    d = (C.c_uint32 * 5)()
    L.pp_defaults(0, 0, 0, d)
    assert list(d) == [workers, workers + beyond, max_batch, min_batch, wait_us]
    L.pp_defaults(2, 0, 4, d)
    assert list(d)[:3] == [2, 2 + beyond, 4]
    L.pp_defaults(2, 7, 0, d)
    assert list(d)[:3] == [2, 7, max_batch]
    assert L.pp_router_depth(workers + beyond, 4) == 4 * (workers + beyond)      # a router: its replicas' depths together
    assert [L.pp_sharded_depth_ok(dp, 8) for dp in (7, 8, 9)] == [0, 1, 1]       # sharded: a full batch must fit among the outstanding


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_core_program_runs_clean_under_the_sanitizers(sanitizer):
    """tests/pipeline_core_main.cpp: the real core over a fake work interface, two ranks per script, 200 seeds — built into a program of
    its own and run on the CPU (nothing is loaded into this interpreter).  It must end, and a run that does not is a failure."""
    exe, stale = build_path("sylph_pipeline_core_" + sanitizer.split(",")[0], [CORE_MAIN, CORE, PLAN])
    if stale:
        tmp = exe + f".{os.getpid()}"
        flags = ["-fsanitize=" + sanitizer] + (["-fno-sanitize-recover=undefined"] if "undefined" in sanitizer else [])
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread"] + flags + ["-Wall", "-Wextra", "-Werror", "-o", tmp, CORE_MAIN])
        os.replace(tmp, exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    if sanitizer == "thread" and p.returncode != 0 and "unexpected memory mapping" in p.stderr and "pipeline core" not in p.stdout:
        pytest.skip("ThreadSanitizer cannot start on this kernel: " + p.stderr.strip().splitlines()[0][:200])
    assert p.returncode == 0 and "pipeline core run ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    assert "x 200 seeds x 2 ranks" in p.stdout
