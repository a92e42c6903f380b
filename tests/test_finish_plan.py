"""CPU tests of the finish loop's plan (sylph_amd/csrc/finish_plan.h, the very header sketch.hip's sketch_finish_impl includes, compiled
with g++ through tests/finish_plan_capi.cpp, which adds a model of what every action can leave behind): every run from every initial
state under every sequence of answers ends, visits no state twice, attempts the bucket path at most once more than it made one-way
transitions, reaches the device-wide replay only on settled marks, a read seeding verdict and records — and the roads the GPU tests
pin by their counters are these action sequences.  Plus the stand-alone sanitizer run."""
import ctypes as C
import os
import subprocess
from collections import namedtuple

import pytest

from .helpers import build_path

HERE = os.path.dirname(os.path.abspath(__file__))
HDR = os.path.join(HERE, "..", "sylph_amd", "csrc", "finish_plan.h")
SRC = os.path.join(HERE, "finish_plan_capi.cpp")

DEFERRED, KNOWN, DENSE = range(3)                                  # Place
NONE, UNREAD, SETTLED = range(3)                                   # Marks
AUTO, GENERIC, BUCKET = range(3)                                   # Mode
NOTHING, DONE, DECLINED, SEEDING_BAD, MARKS_BAD, NEEDS_RECORDS = range(6)   # Outcome
MARK, ATTEMPT, REDO, WALK, RECORDS, READ_SEEDING, READ_FILTER, REPLAY, FAIL = range(9)   # Action
ONE_WAY = (REDO, WALK, RECORDS)            # deferred -> known, partitioned marks -> walk, plain -> records
St = namedtuple("St", "place marks plain filter mode c_lt_2 last")


def word(s):
    return s.place + 3 * s.marks + 9 * s.plain + 18 * s.filter + 36 * s.mode + 108 * s.c_lt_2 + 216 * s.last


def unword(w):
    return St(w % 3, w // 3 % 3, w // 9 % 2, w // 18 % 2, w // 36 % 3, w // 108 % 2, w // 216)


def start(place=DENSE, marks=NONE, plain=0, filter=0, mode=AUTO, c_lt_2=0):
    return St(place, marks, plain, filter, mode, c_lt_2, NOTHING)


@pytest.fixture(scope="module")
def L():
    out, stale = build_path("sylph_finish_plan", [SRC, HDR], ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", tmp, SRC])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    lib.fp_next.argtypes = [C.c_uint32]
    lib.fp_successors.argtypes = [C.c_uint32, C.c_int, C.c_void_p]
    lib.fp_walk_all.argtypes = [C.c_void_p]
    buf = (C.c_uint32 * 16)()

    def successors(s, action):
        n = lib.fp_successors(word(s), action, buf)
        return None if n < 0 else [unword(buf[i]) for i in range(n)]
    lib.successors = successors
    lib.next = lambda s: lib.fp_next(word(s))
    return lib


def all_runs(L, s0):
    """Every run from s0: lists of (state, action) steps; the last step's action is ATTEMPT (answered Done), REPLAY or FAIL."""
    runs = []

    def go(s, steps):
        assert s not in [t for t, _ in steps], ("a state visited twice", steps, s)
        a = L.next(s)
        succ = L.successors(s, a)
        assert succ is not None, ("the action cannot be done in this state", s, a, steps)
        steps = steps + [(s, a)]
        if a in (REPLAY, FAIL):
            runs.append(steps)
            return
        assert succ
        for t in succ:
            if a == ATTEMPT and t.last == DONE:
                runs.append(steps)
            else:
                go(t, steps)
    go(s0, [])
    return runs


def test_every_run_ends_and_attempts_are_bounded_by_the_one_way_transitions(L):
    n_runs, ends, most_attempts, longest = 0, set(), 0, 0
    for w in range(216):
        for run in all_runs(L, unword(w)):
            n_runs += 1
            actions = [a for _, a in run]
            ends.add(actions[-1])
            assert actions[-1] in (ATTEMPT, REPLAY, FAIL) and not set(actions[:-1]) & {REPLAY, FAIL}
            attempts, transitions = actions.count(ATTEMPT), sum(actions.count(a) for a in ONE_WAY)
            assert attempts <= 1 + transitions, run
            assert all(actions.count(a) <= 1 for a in ONE_WAY), run          # each of them at most once: they are one-way
            most_attempts, longest = max(most_attempts, attempts), max(longest, len(run))
            s, last_action = run[-1]
            if last_action == REPLAY:                                       # only on settled marks, a flush that cannot redo the batch, records
                assert (not s.filter or s.marks == SETTLED) and s.place != DEFERRED and not s.plain, run
            if last_action == FAIL:
                assert s.mode == BUCKET, run
            if s.mode == GENERIC or s.c_lt_2:
                assert attempts == 0 and last_action != ATTEMPT, run
            if DECLINED in [t.last for t, _ in run]:                        # a declined attempt is the last one
                first = [t.last for t, _ in run].index(DECLINED)
                assert ATTEMPT not in actions[first:], run
    assert ends == {ATTEMPT, REPLAY, FAIL}
    assert most_attempts == 1 + len(ONE_WAY) == L.fp_max_attempts()         # the bound finish_plan.h states, and a run reaches it
    # the C++ walk of the same runs (what the stand-alone program runs under the sanitizers) saw what this one saw
    out = (C.c_int64 * 8)()
    L.fp_walk_all(out)
    assert out[0] == n_runs and out[4] == 0 and out[5] == most_attempts and out[6] >= 0 and out[7] == longest


def road(L, s0, answers):
    """The actions of one run: `answers` picks, for every action that can leave more than one state behind, the one it leaves (a dict
    of the fields that tell it apart), in order."""
    answers = list(answers)
    s, actions = s0, []
    for _ in range(32):
        a = L.next(s)
        actions.append(a)
        succ = L.successors(s, a)
        assert succ is not None, (s, a)
        if a in (REPLAY, FAIL):
            break
        if len(succ) > 1:
            want = answers.pop(0)
            succ = sorted({t for t in succ if all(getattr(t, k) == v for k, v in want.items())})
        assert len(succ) == 1, (s, a, succ)
        s = succ[0]
        if a == ATTEMPT and s.last == DONE:
            break
    assert not answers
    return actions


PART = dict(marks=UNREAD)                    # Mark chose the partitioned pass
GOOD = dict(last=DONE, plain=0)


def test_roads_the_gpu_tests_pin(L):
    deferred_pairs = start(place=DEFERRED, filter=1)
    # (deferred, deferred_redo, a10_part, a10_redo) = (1, 0, 1, 0): one mark, one attempt, one host round trip
    assert road(L, deferred_pairs, [PART, GOOD]) == [MARK, ATTEMPT]
    assert road(L, start(place=KNOWN, filter=1), [PART, GOOD]) == [MARK, ATTEMPT]
    assert road(L, start(place=DENSE, filter=1), [PART, GOOD]) == [MARK, ATTEMPT]
    assert road(L, deferred_pairs, [dict(marks=SETTLED), GOOD]) == [MARK, ATTEMPT]                 # a10 = walk: (1, 0, 0, 0)
    # (1, 1, 2, 0): the seeding verdict was bad — batch redone, marked again (the marks went with the slots), second attempt
    assert road(L, deferred_pairs, [PART, dict(last=SEEDING_BAD), dict(place=KNOWN), PART, GOOD]) == [MARK, ATTEMPT, REDO, MARK, ATTEMPT]
    # (1, 0, 1, 1): 3,000 copies of one pair — the filter verdict was bad, the walk leaves the sample dense, second attempt
    assert road(L, deferred_pairs, [PART, dict(last=MARKS_BAD), GOOD]) == [MARK, ATTEMPT, WALK, ATTEMPT]
    # both verdicts bad: the seeding verdict first, the filter verdict of the redone batch next
    assert road(L, deferred_pairs, [PART, dict(last=SEEDING_BAD), dict(place=KNOWN), PART, dict(last=MARKS_BAD), GOOD]) == \
        [MARK, ATTEMPT, REDO, MARK, ATTEMPT, WALK, ATTEMPT]
    # the exact set on a deferred batch: nothing but the attempt; its bad verdict: redo and a second one
    assert road(L, start(place=DEFERRED), [GOOD]) == [ATTEMPT]
    assert road(L, start(place=DEFERRED), [dict(last=SEEDING_BAD), dict(place=DENSE), GOOD]) == [ATTEMPT, REDO, ATTEMPT]
    # finish = generic with the filter: the marks are settled without the bucket path
    assert road(L, start(place=DENSE, filter=1, mode=GENERIC), [PART, dict(marks=SETTLED)]) == [MARK, READ_FILTER, REPLAY]
    assert road(L, start(place=DENSE, filter=1, mode=GENERIC), [PART, dict(last=MARKS_BAD)]) == [MARK, READ_FILTER, WALK, REPLAY]
    assert road(L, start(place=DENSE, filter=1, mode=GENERIC), [dict(marks=SETTLED)]) == [MARK, REPLAY]
    # ... also when the option changed behind a deferred push: the seeding verdict before the filter verdict
    assert road(L, start(place=DEFERRED, filter=1, mode=GENERIC), [PART, dict(place=KNOWN, marks=UNREAD), dict(marks=SETTLED)]) == \
        [MARK, READ_SEEDING, READ_FILTER, REPLAY]
    assert road(L, start(place=DEFERRED, filter=1, mode=GENERIC), [PART, dict(place=DENSE, marks=NONE), PART, dict(marks=SETTLED)]) == \
        [MARK, READ_SEEDING, MARK, READ_FILTER, REPLAY]
    assert road(L, start(place=DEFERRED, mode=GENERIC), [dict(place=KNOWN, marks=NONE)]) == [READ_SEEDING, REPLAY]
    # c = 1: the bucket path is never asked; the device-wide replay runs on settled marks
    assert road(L, start(place=DENSE, filter=1, c_lt_2=1), [PART, dict(marks=SETTLED)]) == [MARK, READ_FILTER, REPLAY]
    assert road(L, start(place=DENSE, c_lt_2=1), []) == [REPLAY]
    # a sample the bucket path declines: the device-wide replay, or the refusal of finish = bucket
    assert road(L, start(place=KNOWN), [dict(last=DECLINED)]) == [ATTEMPT, REPLAY]
    assert road(L, start(place=KNOWN, mode=BUCKET), [dict(last=DECLINED)]) == [ATTEMPT, FAIL]
    assert road(L, start(place=DENSE, filter=1, mode=BUCKET, c_lt_2=1), [PART]) == [MARK, FAIL]
    assert road(L, start(place=DENSE, plain=1), [dict(last=DECLINED, plain=1)]) == [ATTEMPT, RECORDS, REPLAY]
    # a marker-less sample with a k-mer deeper than the count kernels take: records after all, second attempt
    assert road(L, start(place=DENSE, plain=1), [dict(last=NEEDS_RECORDS), GOOD]) == [ATTEMPT, RECORDS, ATTEMPT]
    assert road(L, start(place=DENSE, plain=1, mode=GENERIC), []) == [RECORDS, REPLAY]


def test_standalone_program_runs_clean_under_the_sanitizers():
    """tests/finish_plan_sanitize_main.cpp + the model, built with AddressSanitizer and UBSan into a program of its own and run on the
    CPU: nothing is loaded into this interpreter."""
    srcs = [os.path.join(HERE, "finish_plan_sanitize_main.cpp"), SRC]
    exe, stale = build_path("sylph_finish_plan_sanitize", srcs + [HDR])
    if stale:
        tmp = exe + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                               "-Werror", "-o", tmp] + srcs)
        os.replace(tmp, exe)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "finish plan sanitize run ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    assert " 0 runs" not in p.stdout and "at most 4 attempts" in p.stdout
