"""GPU tests of sylph_db_reassign_edges (the reassignment log of `profile --log-reassignments`): every case against a direct
restatement of winner_table and its edge count (contain.rs:410-449) with dictionaries."""
import numpy as np
import pytest

import sylph_amd as S
from oracle import oracle as O

from .test_gpu_parity import BOUNDARY_JS, boundary_db, flat_db

pytestmark = pytest.mark.gpu


def expected_edges(genomes, tracked, passing, ani, lists=None, min_count=1):
    """contain.rs:410-430: a k-mer belongs to the first passing genome with the highest ANI among those that hold it in genome_kmers
    or in the tracked k-mers; :440-449: every occurrence in list i whose owner is another rank counts for (owner, i).
    -> [(winner, loser, count)] sorted by (loser, winner), counts >= max(1, min_count)"""
    winner = {}
    for r, g in enumerate(passing):
        for km in genomes[g].tolist() + tracked[g].tolist():
            if km not in winner or ani[r] > winner[km][0]:
                winner[km] = (ani[r], r)
    edges = {}
    for i, g in enumerate(passing):
        for km in (genomes[g] if lists is None else lists[i]).tolist():
            w = winner.get(km)
            if w is not None and w[1] != i:
                edges[(i, w[1])] = edges.get((i, w[1]), 0) + 1
    return [(w, l, c) for (l, w), c in sorted(edges.items()) if c >= max(1, min_count)]


def edges_of(db, genomes, passing, ani, lists=None, min_count=1):
    lists = [genomes[g] for g in passing] if lists is None else lists
    k, off = flat_db(lists) if len(lists) else (np.zeros(0, dtype=np.uint64), np.zeros(1, dtype=np.uint64))
    w, l, c = db.reassign_edges(k, off, passing, ani, min_count=min_count)
    got = list(zip(w.tolist(), l.tolist(), c.tolist()))
    assert got == sorted(got, key=lambda e: (e[1], e[0]))                  # returned sorted by (loser, winner)
    assert len(set((e[0], e[1]) for e in got)) == len(got)
    return got


def open_db(ctx, genomes, tracked):
    db = S.Database(ctx, *flat_db(genomes))
    if tracked is not None:
        db.attach_tracked(*flat_db(tracked))
    return db


def small_db(rng):
    """The 14 genomes of test_reassign_on_device_matches_reference_semantics: shared genome_kmers, a tracked set that steals, an
    empty tracked set, duplicate postings."""
    pool = np.unique(rng.integers(0, O.threshold(200), size=40000, dtype=np.uint64))
    G = 14
    genomes = [rng.choice(pool, size=int(n), replace=False) for n in rng.integers(300, 3000, size=G)]
    tracked = [rng.choice(pool, size=int(n), replace=False) for n in rng.integers(0, 400, size=G)]
    genomes[2][:500] = genomes[1][:500]
    genomes[5][:300] = genomes[1][200:500]
    tracked[7][:100] = genomes[1][:100]
    tracked[3] = np.zeros(0, dtype=np.uint64)
    genomes[9] = np.concatenate([genomes[9], genomes[9][:50]])
    return pool, genomes, tracked


def test_edges_of_the_small_database(ctx):
    rng = np.random.default_rng(99)
    _, genomes, tracked = small_db(rng)
    db = open_db(ctx, genomes, tracked)
    n_edges = 0
    for trial in range(4):
        passing = rng.permutation(len(genomes))[: int(rng.integers(2, len(genomes) + 1))]
        ani = rng.choice([0.95, 0.96, 0.97, 0.97, 0.99], size=len(passing))          # plenty of ties
        for min_count in (1, 11):
            want = expected_edges(genomes, tracked, passing, ani, min_count=min_count)
            assert edges_of(db, genomes, passing, ani, min_count=min_count) == want, (trial, min_count)
            n_edges += len(want)
    assert n_edges > 20
    passing, ani = np.arange(len(genomes)), np.full(len(genomes), 0.97)              # all tied: the first in the list owns everything shared
    assert edges_of(db, genomes, passing, ani, min_count=0) == expected_edges(genomes, tracked, passing, ani) != []
    db.close()


def test_sizes_at_the_workgroup_edge_and_the_threshold(ctx):
    rng = np.random.default_rng(7)
    pool = np.unique(rng.integers(0, O.threshold(200), size=3000, dtype=np.uint64))
    rng.shuffle(pool)
    core, own = pool[:200], pool[200:]
    g4_own = own[200:257]
    genomes = [np.zeros(0, dtype=np.uint64), core[:1].copy(), np.concatenate([core, own[:55]]), np.concatenate([core, own[100:156]]),
               np.concatenate([core, g4_own]), np.concatenate([g4_own[:10], own[300:340]]), np.concatenate([g4_own[10:21], own[400:440]]),
               own[500:600].copy()]
    assert [len(g) for g in genomes[:5]] == [0, 1, 255, 256, 257]
    tracked = [np.zeros(0, dtype=np.uint64)] * len(genomes)
    db = open_db(ctx, genomes, tracked)
    passing = np.array([5, 6, 2, 3, 4, 1, 0])                                         # genome 7 does not pass
    ani = np.array([0.99, 0.99, 0.98, 0.97, 0.96, 0.95, 0.94])
    want1 = expected_edges(genomes, tracked, passing, ani)
    assert (0, 4, 10) in want1 and (1, 4, 11) in want1 and (2, 4, 200) in want1 and (2, 3, 200) in want1 and (2, 5, 1) in want1
    assert edges_of(db, genomes, passing, ani) == want1
    want11 = [e for e in want1 if e[2] >= 11]
    assert (1, 4, 11) in want11 and not any(e[:2] == (0, 4) for e in want11)          # exactly 11 stays, exactly 10 goes
    assert edges_of(db, genomes, passing, ani, min_count=11) == want11
    # foreign k-mers in a list — one the database does not hold, one only a non-passing genome holds — add nothing
    lists = [genomes[g] for g in passing]
    lists[4] = np.concatenate([lists[4], np.array([int(pool.max()) + 12345], dtype=np.uint64), genomes[7][:3]])
    assert edges_of(db, genomes, passing, ani, lists=lists) == want1
    # a k-mer repeated inside one list counts once per occurrence
    lists[4] = np.concatenate([genomes[4], g4_own[:10]])
    assert (0, 4, 20) in edges_of(db, genomes, passing, ani, lists=lists, min_count=11)
    for g in range(len(genomes)):                                                     # one passing genome: nobody to lose to
        assert edges_of(db, genomes, np.array([g]), np.array([0.97])) == []
    assert edges_of(db, genomes, np.zeros(0, dtype=np.uint32), np.zeros(0)) == []     # n_passing == 0
    db.close()


def test_long_overflow_runs_in_both_indexes(ctx):
    """The 460-strain shared-core database of test_reassign_with_kmers_shared_by_hundreds_of_genomes and the two boundary databases:
    overflow runs around LONG_RUN_MIN and the 64-entry step, walked by the whole wavefront, in the kept and the tracked index."""
    rng = np.random.default_rng(123)
    thr = O.threshold(200)
    core = np.unique(rng.integers(0, thr, size=250, dtype=np.uint64))
    tcore = np.unique(rng.integers(0, thr, size=120, dtype=np.uint64))
    genomes, tracked = [], []
    for g in range(460):
        if g < 400:
            genomes.append(np.concatenate([core[rng.random(len(core)) < 0.95], rng.integers(0, thr, size=20, dtype=np.uint64)]))
            tracked.append(np.concatenate([tcore[rng.random(len(tcore)) < 0.9], core[rng.random(len(core)) < 0.05]]))
        else:
            genomes.append(np.concatenate([rng.integers(0, thr, size=200, dtype=np.uint64), tcore[:30], core[:5]]))
            tracked.append(np.zeros(0, dtype=np.uint64))
    cases = [(genomes, tracked, 250)]
    for extremes in (False, True):
        gb, _ = boundary_db(extremes)
        cases.append((gb, [np.array([j << 40 for j in BOUNDARY_JS if j <= g and (g + j) % 3 == 0], dtype=np.uint64) for g in range(len(gb))], 100))
    for genomes, tracked, min_passing in cases:
        db = open_db(ctx, genomes, tracked)
        for trial in range(2):
            passing = rng.permutation(len(genomes))[: int(rng.integers(min_passing, len(genomes) + 1))]
            ani = rng.choice([0.95, 0.96, 0.97, 0.97, 0.99], size=len(passing)) if trial else np.full(len(passing), 0.97)
            want = expected_edges(genomes, tracked, passing, ani)
            assert len(want) >= min_passing - 10
            assert edges_of(db, genomes, passing, ani) == want
        db.close()


def test_several_windows_equal_one(ctx):
    """300 passing genomes with the window lowered to 64 and to 63 ranks: five windows per loser, winners on both sides of every
    window edge — ranks 63, 64 and 65 hold the highest ANIs and win most of the shared core."""
    rng = np.random.default_rng(300)
    thr = O.threshold(200)
    core = np.unique(rng.integers(0, thr, size=60, dtype=np.uint64))
    genomes = [np.concatenate([core[rng.random(len(core)) < 0.5], rng.integers(0, thr, size=30, dtype=np.uint64)]) for _ in range(300)]
    tracked = [core[rng.random(len(core)) < 0.1] for _ in range(300)]
    passing = rng.permutation(300)
    ani = rng.choice([0.95, 0.96, 0.97], size=300)
    ani[[63, 64, 65, 127, 128, 299, 0]] = [0.999, 0.998, 0.997, 0.996, 0.995, 0.994, 0.993]
    want = expected_edges(genomes, tracked, passing, ani)
    for w in (63, 64, 65):
        assert sum(1 for e in want if e[0] == w) > 5
    db = open_db(ctx, genomes, tracked)
    try:
        for window in ("8192", "64", "63", "1"):
            ctx.set_option("reassign_edge_window", window)
            assert edges_of(db, genomes, passing, ani) == want, window
            assert edges_of(db, genomes, passing, ani, min_count=11) == [e for e in want if e[2] >= 11], window
        with pytest.raises(S.SylphHipError):
            ctx.set_option("reassign_edge_window", "8193")
    finally:
        ctx.set_option("reassign_edge_window", "8192")
        db.close()


def test_more_edges_than_the_first_list_holds(ctx):
    """400 passing genomes, one k-mer per pair of them: 79,800 edges of count 1, more than the 2^16 the first count launch has room
    for — the launch is repeated once with room for all."""
    n = 400
    a, b = np.triu_indices(n, 1)
    pair_km = (np.arange(len(a), dtype=np.uint64) + np.uint64(1)) * np.uint64(1000003)
    genomes = [np.concatenate([pair_km[a == g], pair_km[b == g]]) for g in range(n)]
    tracked = [np.zeros(0, dtype=np.uint64)] * n
    passing = np.arange(n)
    ani = np.linspace(0.99, 0.95, n)                                                  # the lower rank of a pair wins its k-mer
    db = open_db(ctx, genomes, tracked)
    w, l, c = db.reassign_edges(*flat_db(genomes), passing, ani, min_count=1)
    assert len(w) == n * (n - 1) // 2 > 2**16 and (c == 1).all()
    order = np.lexsort((a, b))
    assert np.array_equal(w, a[order]) and np.array_equal(l, b[order])
    assert len(db.reassign_edges(*flat_db(genomes), passing, ani, min_count=2)[0]) == 0
    db.close()


def test_edge_counts_add_up_to_kmers_lost(ctx):
    """Against the reassignment pass itself: with a sample that holds every database k-mer once, a passing genome's kmers_lost is the
    sum of the edges that point at it."""
    rng = np.random.default_rng(99)
    _, genomes, tracked = small_db(rng)
    db = open_db(ctx, genomes, tracked)
    sk = np.unique(np.concatenate(genomes))
    for trial in range(3):
        passing = rng.permutation(len(genomes))[: int(rng.integers(3, len(genomes) + 1))]
        ani = rng.choice([0.95, 0.96, 0.97, 0.97, 0.99], size=len(passing))
        w, l, c = db.reassign_edges(*flat_db([genomes[g] for g in passing]), passing, ani, min_count=1)
        _, _, _, lost = db.reassign_view(sk, np.ones(len(sk), dtype=np.uint32), passing, ani)
        per_loser = np.bincount(l, weights=c, minlength=len(passing)).astype(np.int64)
        assert per_loser.sum() > 100
        for r, g in enumerate(passing):
            assert per_loser[r] == lost[g], (trial, r, g)
    db.close()


def test_borrowed_views_survive_the_call(ctx):
    rng = np.random.default_rng(99)
    pool, genomes, tracked = small_db(rng)
    db = open_db(ctx, genomes, tracked)
    sk = np.sort(rng.choice(pool, size=25000, replace=False))
    sc = rng.integers(0, 6, size=len(sk)).astype(np.uint32)
    cc, off, covs = db.contain_view(sk, sc, min_number_kmers=0.0)
    before = (cc.copy(), off.copy(), covs.copy())
    assert before[0].sum() > 1000
    passing = np.arange(len(genomes))
    assert len(edges_of(db, genomes, passing, rng.choice([0.95, 0.97, 0.99], size=len(passing)))) > 5
    for view, copy in zip((cc, off, covs), before):
        assert np.array_equal(view, copy)
    db.close()


def test_errors(ctx):
    rng = np.random.default_rng(99)
    _, genomes, tracked = small_db(rng)
    db = open_db(ctx, genomes, tracked)
    k, off = flat_db([genomes[1], genomes[2]])
    want = expected_edges(genomes, tracked, [1, 2], [0.99, 0.95])
    assert len(want) == 1 and want[0][:2] == (0, 1) and want[0][2] >= 500
    assert edges_of(db, genomes, np.array([1, 2]), np.array([0.99, 0.95])) == want
    with pytest.raises(S.SylphHipError):
        db.reassign_edges(k, off, [1, 1], [0.99, 0.95])                               # listed twice
    with pytest.raises(S.SylphHipError):
        db.reassign_edges(k, off, [1, len(genomes)], [0.99, 0.95])                    # out of range
    with pytest.raises(S.SylphHipError):
        db.reassign_edges(k, np.array([0, len(k), len(genomes[1])], dtype=np.uint64), [1, 2], [0.99, 0.95])   # kmer_off decreases
    w, l, c = db.reassign_edges(np.zeros(0, dtype=np.uint64), np.zeros(1, dtype=np.uint64), [], [])
    assert len(w) == len(l) == len(c) == 0 and w.dtype == np.uint32
    db.close()
    dbk, goff = flat_db(genomes)
    shard = S.Database(ctx, dbk, goff, shard=(S.shard_bounds(int(dbk.max()), 2), 2, 0))   # one k-mer-range shard of two
    with pytest.raises(S.SylphHipError):
        shard.reassign_edges(k, off, [1, 2], [0.99, 0.95])
    shard.close()
