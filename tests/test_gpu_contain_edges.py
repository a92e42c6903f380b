"""Containment ON its thresholds (inputs: tests/contain_edges.py, proved on the CPU by tests/test_contain_edges_inputs.py): values at
4095 / 4096 (hits.hip MAX_VALUE_LDS: row assembly or sorted finish, decided on the device and on the host) and at the width edges,
rows of 63 .. 65, 255 .. 257 and 4095 .. 4097 hits, row counts around the 2048-row tile and more than 256 tiles, batches of more than
8 tables (descriptors in HBM), compact 32-bit sort keys at cb + rb = 32 / 33, genome ids at and past a power of two with run lengths
that saturate the descriptor, reassignment with wide counts, and one database through all of these in turn.  Everything is compared
bit for bit with the expectation by construction and with the oracle; a child process repeats it with the sorted finish forced."""
import contextlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import sylph_amd as S

from . import contain_edges as E
from .test_gpu_parity import assert_reassigned, check_reassign, flat_db

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@contextlib.contextmanager
def profiled(ctx):
    ctx.profile(True)
    try:
        yield
    finally:
        ctx.profile(False)


@contextlib.contextmanager
def database(ctx, db_kmers, goff, tracked=None):
    db = S.Database(ctx, db_kmers, goff)
    try:
        if tracked is not None:
            db.attach_tracked(*flat_db(tracked))
        yield db
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------------------------- a. rows and values
@pytest.mark.parametrize("pattern", E.PATTERNS)
def test_row_lengths(ctx, pattern):
    """rows of 0, 1, 2, 63 .. 65, 127 .. 129, 255 .. 257, 4095 .. 4097 and 20,000 hits: all values equal (the wavefront ranking's tie rule),
    strictly descending in table order, two alternating values, random"""
    case = E.row_lengths_case(pattern)
    E.assert_oracle(case, 0.0)
    with profiled(ctx), database(ctx, case.db_kmers, case.goff) as db:
        narrow = E.check_single(ctx, db, case, 0.0)
    assert narrow == {"equal": np.uint8, "alternating": np.uint8}.get(pattern, np.uint16)


def test_batch_maxima(ctx):
    """the largest count among the hits at 1, 255, 256, 4095, 4096, 65535, 65536 and 3,000,000,000, in a 65-hit row and in a 1-hit row:
    u8 / u16 / u32 values, row assembly up to 4095 and the sorted finish from 4096 (path_checked)"""
    cases = {name: build() for name, build in E.ladder_cases().items() if name.startswith("max_") and name != "max_outside_the_hits"}
    first = next(iter(cases.values()))
    assert len(cases) == 16 and all(np.array_equal(c.db_kmers, first.db_kmers) for c in cases.values())
    with profiled(ctx), database(ctx, first.db_kmers, first.goff) as db:
        for name, case in cases.items():
            E.assert_oracle(case, 0.0)
            m = int(name.split("_")[1])
            assert E.check_single(ctx, db, case, 0.0) == (np.uint8 if m <= 255 else np.uint16 if m <= 65535 else np.uint32), name
    case = E.outside_max_case()                                   # the sample's 3,000,000,000 is no hit: one-byte values, no sort
    E.assert_oracle(case, 0.0)
    with profiled(ctx), database(ctx, case.db_kmers, case.goff) as db:
        assert E.check_single(ctx, db, case, 0.0) == np.uint8


# ------------------------------------------------------------------------------------------------------------------- b. row counts
@pytest.mark.parametrize("G", E.TINY_G)
def test_row_count_edges(ctx, G):
    """G and 3 G rows around the tile (2048) and counter (1024, powers of two) sizes; genome ids at and past a power of two; at
    G = 65535 / 65536 with a hit of count 65535 in the last row the sorted finish takes 32-bit keys that use every bit / 64-bit keys"""
    db_kmers, goff, _ = E.tiny_db(G)
    singles = [E.tiny_case(G, v) for v in (0, 1, 2)]
    with profiled(ctx), database(ctx, db_kmers, goff) as db:
        for case in singles:
            E.assert_oracle(case, 0.0)
            E.check_single(ctx, db, case, 0.0)
        E.check_batch(ctx, db, E.stack_cases(singles), 0.0, device=False)
        if G >= 65535:
            top = E.tiny_case(G, 0, top=65535)
            E.assert_oracle(top, 0.0)
            assert top.expected_sorted_vectors[G - 1][-1] == 65535
            assert E.check_single(ctx, db, top, 0.0) == (np.uint16 if G == 65535 else np.uint32)
            assert E.check_batch(ctx, db, E.stack_cases([singles[1], top, singles[2]]), 0.0, device=False) == np.uint32   # 3 G rows: rb = 18


# ------------------------------------------------------------------------------------------------------------------- c. batches
@pytest.mark.parametrize("n_tables", E.BATCH_S)
def test_batches(ctx, n_tables):
    """8, 9, 16, 33, 64 and 65 tables in one launch (above 8 the probe reads the table descriptors from HBM and searches them for the
    chunk's table): sizes 0, 1, 511 .. 513, 1025 and thousands, empty tables first, in the middle and last, host and device resident"""
    kinds = ["mixed"] + (["wide"] if n_tables in (9, 64) else []) + (["empty"] if n_tables == 9 else [])
    db_kmers, goff = E.batch_db()[3:]
    with profiled(ctx), database(ctx, db_kmers, goff) as db:
        for kind in kinds:
            case = E.batch_case(n_tables, kind)
            E.assert_oracle(case, E.BATCH_MIN_KMERS)
            narrow = E.check_batch(ctx, db, case, E.BATCH_MIN_KMERS, singles=kind == "mixed")
            assert narrow == {"mixed": np.uint16, "wide": np.uint32, "empty": np.uint8}[kind]


def test_many_tiles(ctx):
    """64 tables x 8193 genomes = 524,352 rows = 257 tiles: rows_scan_kernel's 256 threads add the tile totals in two steps.  Every
    contain_count, every offset, every coverage vector."""
    case = E.many_tiles_case()
    E.assert_oracle(case, 0.0)
    with profiled(ctx), database(ctx, case.db_kmers, case.goff) as db:
        assert E.check_batch(ctx, db, case, 0.0, singles=False, device=False) == np.uint8


def test_too_many_rows_are_refused_before_any_launch(ctx):
    """70,000 (empty) tables x 65,536 genomes >= 2^32 - 1 rows: refused by the argument check; the next call is right"""
    case = E.tiny_case(65536, 0)
    empty = (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    with profiled(ctx), database(ctx, case.db_kmers, case.goff) as db:
        E.check_single(ctx, db, case, 0.0)
        before = [ctx.kernel_stats(f)[1] for f in ("probe", "assemble", "sort")]
        with pytest.raises(S.SylphHipError, match="too many result rows|samples x genomes"):
            db.contain_batch([empty] * 70_000, min_number_kmers=0.0)
        assert [ctx.kernel_stats(f)[1] for f in ("probe", "assemble", "sort")] == before
        E.check_single(ctx, db, case, 0.0)
        E.check_batch(ctx, db, E.stack_cases([case, E.tiny_case(65536, 1)]), 0.0, device=False)


# ------------------------------------------------------------------------------------------------------------------- d. genome ids
@pytest.mark.parametrize("G", E.SHARED_G)
def test_genome_id_edges(ctx, G):
    """a key every genome holds (once and three times) with 40 neighbours in its bucket: G = 1, 2 (gb clamped to 1), G at and past a
    power of two (the largest id is all ones beside the descriptor flag), run lengths that saturate the descriptor below LONG_RUN_MIN
    (G <= 32: one lane walks the run) and at 63 (G 33 .. 64: the wavefront does), short genomes filtered inside the run"""
    with profiled(ctx):
        for r in (1, 3):
            for short in (False, True):
                d = E.shared_key_db(G, r, short)
                with database(ctx, *flat_db(d.genomes)) as db:
                    for min_kmers in (0.0, 5.0):
                        case = E.shared_key_case(G, r, short, min_kmers)
                        E.assert_oracle(case, min_kmers)
                        E.check_single(ctx, db, case, min_kmers)
                        cc, off, covs = db.contain(case.sample_kmers, case.sample_counts, min_number_kmers=min_kmers)
                        for g in range(G):
                            gone = d.short[g] and min_kmers == 5.0
                            assert cc[g] == (0 if gone else r + (E.NEIGHBOURS if d.holders[g] else 0) + (1 if d.short[g] else 3)), (r, short, g)
                            assert gone or int((covs[int(off[g]):int(off[g + 1])] == E.SHARED_COUNT).sum()) >= r


# ------------------------------------------------------------------------------------------------------------------- e. reassignment
def reassign_path_checked(ctx, db, sk, sc, passing, ani, wide):
    before = ctx.kernel_stats("sort")[1]
    result = tuple(np.array(a) for a in db.reassign_view(sk, sc, passing, ani))
    assert (ctx.kernel_stats("sort")[1] > before) == wide
    return result


@pytest.mark.parametrize("cap", [255, 256, 4095, 4096, 65536, 3_000_000_000])
def test_reassignment_with_wide_counts(ctx, cap):
    """finish_driver (with_lost) with a host-known largest count below and from 4096: kmers_lost sits behind a block whose layout follows
    the path and the width"""
    genomes, tracked, sk, sc = E.shared_core_db(cap)
    rng = np.random.default_rng(cap % 1000)
    check_reassign(ctx, genomes, tracked, sk, sc, rng, min_passing=30, min_lost=1000)
    smap = dict(zip(sk.tolist(), sc.tolist()))
    with profiled(ctx), database(ctx, *flat_db(genomes), tracked=tracked) as db:
        for passing, ani in ((rng.permutation(60), rng.choice([0.95, 0.97, 0.97, 0.99], size=60)), (rng.permutation(60)[:31], np.full(31, 0.97))):
            result = reassign_path_checked(ctx, db, sk, sc, passing, ani, wide=cap >= E.MAX_VALUE_LDS)
            assert_reassigned(result, genomes, tracked, smap, passing, ani)
            assert int(result[2].max()) == cap                  # every passing genome keeps its own key of count `cap`


@pytest.mark.parametrize("G", [1, 2, 33, 64, 65])
def test_reassignment_all_tied_over_a_shared_key(ctx, G):
    """every genome passes with the same ANI: the shared key goes to the first of the passing list, its neighbours to the first holder
    — kept vectors and kmers_lost by construction"""
    d = E.shared_key_db(G, 3)
    none = [np.zeros(0, dtype=np.uint64)] * G
    rng = np.random.default_rng(G)
    check_reassign(ctx, d.genomes, none, d.sample_kmers, d.sample_counts, rng, min_passing=G, min_lost=-1)
    with profiled(ctx), database(ctx, *flat_db(d.genomes), tracked=none) as db:
        for passing in (rng.permutation(G), np.arange(G)[::-1].copy()):
            cc, off, covs, lost = reassign_path_checked(ctx, db, d.sample_kmers, d.sample_counts, passing, np.full(G, 0.97), wide=False)
            vectors, want_lost = E.shared_key_tied_reassignment(d, passing)
            assert np.array_equal(lost, want_lost) and np.array_equal(cc, [len(v) for v in vectors])
            assert np.array_equal(covs, np.concatenate(vectors)) and np.array_equal(np.diff(off.astype(np.int64)), cc)
            assert int(lost.sum()) == 3 * (G - 1) + E.NEIGHBOURS * (sum(d.holders) - 1)


# ------------------------------------------------------------------------------------------------------------------- f. one database
def test_one_database_through_every_road(ctx):
    """rc_dirty / rc_rows / cnt_dirty and the buffers hits_sorted, res and row_meta carried from call to call: row path, reassignment on
    the sorted path, 64 tables, a single sample at 4096, an empty one, 9 tables, reassignment on the row path, a single sample at 4095 —
    each result equal to the same call on a fresh database"""
    pool, shared, cluster, db_kmers, goff = E.batch_db()
    G = len(goff) - 1
    rng = np.random.default_rng(66)
    tracked = [rng.choice(pool, size=30, replace=False) if g % 2 else np.zeros(0, dtype=np.uint64) for g in range(G)]
    b64, b9 = E.batch_tables(64), E.batch_tables(9)
    k, c = b9[5]
    assert len(k) > 500 and int(c.max()) < 300 and k[0] == shared[0]

    def with_count(value):
        c2 = c.copy()
        c2[0] = value                                          # shared[0]: a hit in (almost) every genome
        return c2
    passing, ani = rng.permutation(G)[:200], rng.choice([0.95, 0.97, 0.97, 0.99], size=200)
    roads = [("row path", lambda d: d.contain_view(k, c, packed=True)),
             ("reassign, 70,000", lambda d: d.reassign_view(k, with_count(70_000), passing, ani)),
             ("64 tables", lambda d: d.contain_batch(b64)),
             ("max 4096", lambda d: d.contain_view(k, with_count(4096), packed=True)),
             ("empty sample", lambda d: d.contain_view(k[:0], c[:0], packed=True)),
             ("9 tables", lambda d: d.contain_batch(b9)),
             ("reassign, small", lambda d: d.reassign_view(k, c, passing, ani)),
             ("max 4095", lambda d: d.contain_view(k, with_count(4095), packed=True))]
    with database(ctx, db_kmers, goff, tracked=tracked) as db:
        carried = [tuple(np.array(a) for a in road(db)) for _, road in roads]
    for (name, road), got in zip(roads, carried):
        with database(ctx, db_kmers, goff, tracked=tracked) as fresh:
            want = tuple(np.array(a) for a in road(fresh))           # (copies: the views die with the database)
            assert len(want) == len(got) and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want)), name
    genomes = [db_kmers[int(goff[g]):int(goff[g + 1])] for g in range(G)]
    for i, counts in ((1, with_count(70_000)), (6, c)):
        assert_reassigned(carried[i], genomes, tracked, dict(zip(k.tolist(), counts.tolist())), passing, ani, roads[i][0])
    assert carried[0][2].dtype == np.uint16 and carried[3][2].dtype == np.uint16 and int(carried[3][2].max()) == 4096 and int(carried[7][2].max()) == 4095
    assert int(carried[1][2].max()) == 70_000 and carried[4][0].sum() == 0 and len(carried[2][0]) == 64 * G


# ------------------------------------------------------------------------------------------------------------------- the sorted finish, forced
WORKER_SECONDS = 5.6       # the child's wall time measured on an MI355X (start-up, torch and the library included)
WORKER_TIMEOUT = 5 * WORKER_SECONDS   # x 5: a busy shared machine must not trip it


def test_sorted_finish_forced_on_ordinary_inputs():
    """SYLPH_HIP_HIT_SORT is read once per process: one fresh child (tests/contain_edges_worker.py) runs the ladder cases, the row-count
    edges up to 4097 genomes and the 9- and 64-table batches through finish_hits_sorted"""
    env = dict(os.environ, SYLPH_HIP_HIT_SORT="1")
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "tests.contain_edges_worker"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=WORKER_TIMEOUT)
    print(f"contain_edges_worker: {time.time() - t0:.1f} s")
    assert r.returncode == 0 and "contain edges sorted ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
