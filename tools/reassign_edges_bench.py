#!/usr/bin/env python3
"""Times sylph_db_reassign_edges (the reassignment log) and its two launches, beside sylph_db_reassign_view on a sample of as many
k-mers on the same database, and beside the same edge count done on the host with numpy (a sort in place of the reference's hash
map).  Two shapes: the fixture of tests/test_gpu_cli_reassign_log.py, and a synthetic 1,000 passing genomes x 20,000 k-mers
against a 10,000-genome database (100 species of 100 strains, 90 % of a strain's k-mers its species' core).
Usage: python tools/reassign_edges_bench.py [--genomes 10000 --kmers 20000 --passing 1000 --reps 5]   (prints; profiles/reassign_edges.txt)"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import sylph_amd as S  # noqa: E402


def host_edges(lists, ani, min_count):
    """winner = highest ANI, ties to the lowest rank; count (winner, loser) over every occurrence"""
    k = np.concatenate(lists)
    rank = np.repeat(np.arange(len(lists)), [len(x) for x in lists])
    order = np.lexsort((rank, -ani[rank], k))
    ks, rs = k[order], rank[order]
    first = np.concatenate([[True], ks[1:] != ks[:-1]])
    win_sorted = rs[np.maximum.accumulate(np.where(first, np.arange(len(ks)), 0))]
    winner = np.empty(len(k), dtype=np.int64)
    winner[order] = win_sorted
    lose = winner != rank
    key, cnt = np.unique(rank[lose] * (1 << 32) + winner[lose], return_counts=True)
    return int((cnt >= min_count).sum())


def measure(ctx, tag, genomes, tracked, passing, ani, sample, reps, min_count=11):
    off = np.zeros(len(genomes) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(g) for g in genomes])
    db = S.Database(ctx, np.concatenate(genomes), off)
    if tracked is not None:
        toff = np.zeros(len(tracked) + 1, dtype=np.uint64)
        toff[1:] = np.cumsum([len(t) for t in tracked])
        db.attach_tracked(np.concatenate(tracked), toff)
    lists = [genomes[g] for g in passing]
    k = np.concatenate(lists)
    koff = np.zeros(len(lists) + 1, dtype=np.uint64)
    koff[1:] = np.cumsum([len(x) for x in lists])
    sc = np.ones(len(sample), dtype=np.uint32)
    print(f"== {tag}: {len(genomes)} genomes, {int(off[-1])} postings; {len(passing)} passing, {len(k)} query k-mers; sample of {len(sample)} k-mers")
    n_edges = len(db.reassign_edges(k, koff, passing, ani, min_count=min_count)[0])   # warm-up (buffers, pool)
    db.reassign_view(sample, sc, passing, ani)
    ctx.profile(True)
    t0 = time.perf_counter()
    for _ in range(reps):
        db.reassign_edges(k, koff, passing, ani, min_count=min_count)
    wall = (time.perf_counter() - t0) / reps * 1e3
    w_ms, w_n = ctx.kernel_stats("edge_winner")
    c_ms, c_n = ctx.kernel_stats("edge_count")
    print(f"sylph_db_reassign_edges (host k-mers in, {n_edges} edges >= {min_count} out): {wall:.3f} ms per call; edge_winner {w_ms / max(1, w_n):.3f} ms, "
          f"edge_count {c_ms / max(1, c_n):.3f} ms per launch ({int(w_n)} + {int(c_n)} launches)")
    ctx.profile(True)
    t0 = time.perf_counter()
    for _ in range(reps):
        db.reassign_view(sample, sc, passing, ani)
    wall = (time.perf_counter() - t0) / reps * 1e3
    p_ms, p_n = ctx.kernel_stats("probe")
    print(f"sylph_db_reassign_view (host sample in, result rows out): {wall:.3f} ms per call; reassign_kernel {p_ms / max(1, p_n):.3f} ms per launch")
    ctx.profile(False)
    t0 = time.perf_counter()
    n_host = host_edges(lists, np.asarray(ani, dtype=np.float64), min_count)
    print(f"host, numpy (sort for the winner table, unique for the edges; tracked k-mers left out): {(time.perf_counter() - t0) * 1e3:.1f} ms, {n_host} edges")
    db.close()


def fixture_case(ctx, reps):
    from oracle import oracle as O
    from tests import test_gpu_cli_reassign_log as T
    d = T.make_data(tempfile.mkdtemp(), os.path.join(ROOT, "tests", "golden"))
    gs = []
    for name in T.ORDER:
        b, off = O.concat([bytes(r[1]) for r in d["genomes"][name][1]])
        gs.append(O.sketch_genome(b, off))
    b, off = O.concat([bytes(x) for p in zip(d["m1"], d["m2"]) for x in p])
    s = O.sketch_reads(b, off, paired=True)
    passing = np.array([0, 1, 4])                                      # EC590, K12 and the constructed strain pass the first pass
    measure(ctx, "CLI test fixture", [g["genome_kmers"] for g in gs], [g["tracked"] for g in gs], passing, np.array([0.999, 1.0, 0.998]), s["kmers"], reps)


def synthetic_case(ctx, n_genomes, n_kmers, n_passing, reps):
    rng = np.random.default_rng(1)
    per_species = 100
    n_core = n_kmers * 9 // 10
    cores = [rng.integers(0, 2**63, size=n_kmers, dtype=np.uint64) for _ in range(-(-n_genomes // per_species))]
    genomes, owns = [], []
    for g in range(n_genomes):
        own = rng.integers(0, 2**63, size=n_kmers - n_core, dtype=np.uint64)
        owns.append(own)
        genomes.append(np.concatenate([rng.choice(cores[g // per_species], size=n_core, replace=False), own]))
    passing = rng.choice(n_genomes // per_species, size=max(1, n_passing // per_species), replace=False)
    passing = rng.permutation(np.concatenate([np.arange(s * per_species, (s + 1) * per_species) for s in passing]))[:n_passing]
    ani = rng.choice(np.linspace(0.95, 1.0, 200), size=len(passing))
    want = sum(len(genomes[g]) for g in passing)
    sample = np.unique(np.concatenate(cores + owns))[:want]
    measure(ctx, "synthetic", genomes, None, passing, ani, sample, reps)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=10000)
    ap.add_argument("--kmers", type=int, default=20000)
    ap.add_argument("--passing", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-fixture", action="store_true")
    a = ap.parse_args()
    ctx = S.Context(0)
    if not a.no_fixture:
        fixture_case(ctx, a.reps)
    synthetic_case(ctx, a.genomes, a.kmers, a.passing, a.reps)
    ctx.close()
