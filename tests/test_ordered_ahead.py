"""CPU tests of the command's hand-over of samples to the pipeline, sylph_amd/host/ordered_ahead.hpp (what `query` / `profile` prepare
ahead, submit and consume with; host/cmd_contain.cpp).  Its decisions, through tests/ordered_ahead_capi.cpp, against the values the
command's two sample loops used before the header took them over; its threads — the pool, the gate, the ordered driver and its
clean-up — in tests/ordered_ahead_main.cpp, a program of its own over a fake pipeline, under ThreadSanitizer and under
AddressSanitizer + UBSan."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from .helpers import build_path

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "sylph_amd", "host", "ordered_ahead.hpp")
SRC = os.path.join(HERE, "ordered_ahead_capi.cpp")
MAIN = os.path.join(HERE, "ordered_ahead_main.cpp")


@pytest.fixture(scope="module")
def L():
    out, stale = build_path("sylph_ordered_ahead", [SRC, HEADER], ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, SRC])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    for f in (lib.oa_ahead_limit, lib.oa_pipeline_depth):
        f.argtypes, f.restype = [C.c_uint64], C.c_uint64
    lib.oa_gate_open.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]
    lib.oa_must_wait.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    return lib


def test_decisions_are_the_sample_loops_own(L):
    """`ahead_limit = n_workers + 2`, a pipeline of `ahead_limit + 1`, the gate `cancel || j < released + ahead_limit` and
    `must_wait = outstanding == 0 && submitted == done`: what both loops of the command spelled out by hand."""
    for w in range(1, 70):
        assert L.oa_ahead_limit(w) == w + 2
        assert L.oa_pipeline_depth(L.oa_ahead_limit(w)) == w + 3
    assert [L.oa_pipeline_depth(a) for a in (3, 5, 10)] == [4, 6, 11]
    for j, released, limit, cancelled in itertools.product(range(12), range(8), (3, 5), (0, 1)):
        assert L.oa_gate_open(j, released, limit, cancelled) == (cancelled or j < released + limit)
    for outstanding, done in itertools.product(range(4), range(5)):
        for submitted in range(done, done + 4):
            assert L.oa_must_wait(outstanding, submitted, done) == (outstanding == 0 and submitted == done)


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_pool_and_driver_run_clean_under_the_sanitizers(sanitizer):
    """tests/ordered_ahead_main.cpp: the real pool and driver over a fake pipeline, 60 cases x 200 seeds — built into a program of its
    own and run on the CPU (nothing is loaded into this interpreter).  It must end, and a run that does not is a failure: the time
    limit is only that cap — the program took 13-27 s where it was written, most of it the prepare functions' sleeps."""
    exe, stale = build_path("sylph_ordered_ahead_" + sanitizer.split(",")[0], [MAIN, HEADER])
    if stale:
        tmp = exe + f".{os.getpid()}"
        flags = ["-fsanitize=" + sanitizer] + (["-fno-sanitize-recover=undefined"] if "undefined" in sanitizer else [])
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread"] + flags + ["-Wall", "-Wextra", "-Werror", "-o", tmp, MAIN])
        os.replace(tmp, exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if sanitizer == "thread" and p.returncode != 0 and "unexpected memory mapping" in p.stderr and "ordered ahead" not in p.stdout:
        pytest.skip("ThreadSanitizer cannot start on this kernel: " + p.stderr.strip().splitlines()[0][:200])
    assert p.returncode == 0 and "ordered ahead run ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    assert "60 cases x 200 seeds" in p.stdout
    assert "Sanitizer" not in p.stderr, p.stderr[-3000:]
