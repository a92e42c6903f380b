"""Worker for tests/test_gpu_shard_worlds.py — run under torch.distributed.run with 3, 5 or 8 ranks, all of them on cuda:0.
Every rank builds the same four small databases from fixed seeds, holds its shard of each under every cut (k-mer ranges with the
library's equal-width bounds, k-mer ranges with hand-made bounds for D1, genome ranges) and runs the same list of steps through
sylph_db_contain_batch_sharded, the collectives going through torch.distributed (gloo) callbacks.  Every step runs under both
"shard_reduce" settings and every cut; every rank compares contain_count of every genome row and every coverage vector of its own
samples with oracle.contain over the WHOLE database.  Rank 0 prints one line per (database, cut, reduce, step).  (With 8 ranks the
list is shorter on D1-D3: PLAN_AT_8 below says which steps and why.)

  D0  ordinary: lengths 0..1500, an empty genome, one of 49 k-mers, repeated k-mers, 300 k-mers shared by 46 genomes
  D1  holes in the key space: everything below 2^40 but one k-mer near 2^62 — middle ranks hold no posting; and hand-made bounds with hi == lo
  D2  five genomes, two of them empty: more ranks than genomes
  D3  D0 + the keys 0 and 2^64 - 1 (+ both sides of every range boundary), in the database and in the samples
"""
import os
import sys
import time

T0 = time.time()

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sylph_amd as S  # noqa: E402
from oracle import oracle as O  # noqa: E402
from sylph_amd import shard as SH  # noqa: E402

U64MAX = 2**64 - 1
MAX_LOCAL = 64                       # shard_plan.h: a 65th sample fails before the first collective and the others would wait
REDUCES = ("alltoall", "allgather")
EMPTY = np.zeros(0, np.uint64)


def u64(x):
    return np.asarray(x, dtype=np.uint64)


def edge_keys(bounds):
    """0, 2^64 - 1 and both sides of every boundary: where lower_bound_u64 decides which rank an entry goes to."""
    b = [int(x) for x in bounds]
    return u64(sorted({0, U64MAX} | set(b) | {x - 1 for x in b if x}))


def d0(world, extreme=False):
    rng = np.random.default_rng(5)
    pool = np.unique(rng.integers(0, O.threshold(200), size=20000, dtype=np.uint64))
    lens = np.concatenate([rng.integers(0, 1500, size=12), rng.integers(0, 500, size=36)])
    lens[5] = 0
    lens[9] = 49
    genomes = [rng.choice(pool, size=int(n), replace=False) for n in lens]
    shared = rng.choice(pool, size=300, replace=False)                # spread over every k-mer range
    for g in range(len(genomes)):
        if g not in (5, 9):
            genomes[g] = np.concatenate([genomes[g], shared])         # 46 genomes hold them (some twice: counted twice)
    genomes[21] = np.concatenate([genomes[21], genomes[21][:10]])     # repeated k-mers
    db = dict(name="D0", pool=pool, genomes=genomes, must=shared, short=9, edges=None, max_key=int(max(g.max() for g in genomes if len(g))))
    if extreme:
        bounds = S.shard_bounds(U64MAX, world)
        edges = edge_keys(bounds)
        genomes[30] = np.concatenate([genomes[30], u64([0, U64MAX])])
        genomes[31] = np.concatenate([genomes[31], edges])            # a boundary key routed to the wrong side is a lost hit
        db.update(name="D3", edges=edges, max_key=U64MAX)
    return db


def d1(world):
    rng = np.random.default_rng(6)
    pool = np.unique(rng.integers(0, 2**40, size=12000, dtype=np.uint64))
    genomes = [rng.choice(pool, size=int(n), replace=False) for n in rng.integers(0, 800, size=20)]
    big = 2**62 + 12345
    genomes[7] = np.concatenate([rng.choice(pool, size=60, replace=False), u64([big])])
    hand = [0, 2**39, 2**39] + [2**39 + (j - 2) * 2**36 for j in range(3, world)] + [big + 1]     # rank 1: hi == lo
    return dict(name="D1", pool=pool, genomes=genomes, must=u64([big]), short=None, edges=None, max_key=big, hand=u64(hand))


def d2(world):
    rng = np.random.default_rng(7)
    pool = np.unique(rng.integers(0, O.threshold(200), size=3000, dtype=np.uint64))
    genomes = [rng.choice(pool, size=300, replace=False), EMPTY, rng.choice(pool, size=200, replace=False),
               rng.choice(pool, size=120, replace=False), EMPTY]
    return dict(name="D2", pool=pool, genomes=genomes, must=EMPTY, short=None, edges=None, max_key=int(max(g.max() for g in genomes if len(g))))


def draw(rng, D, n, must=True, edges=True):
    """An ascending sample table: n keys of the pool (+ the database's shared keys, + D3's edge keys)."""
    parts = [rng.choice(D["pool"], size=n, replace=False)]
    if must:
        parts.append(D["must"])
    if edges and D["edges"] is not None:
        parts.append(D["edges"])
    return np.unique(np.concatenate(parts))


def counts(rng, k, top=9):
    return rng.integers(0, top, size=len(k), dtype=np.int64).astype(np.uint32)


def make_steps(D, di, bounds, rank, world):
    """This rank's part of every step: [(label, samples, options)].  Sizes depend on (rank, world) only, the draws on a per-rank seed."""
    rng = np.random.default_rng(1000 * di + 100 + rank)
    mid, last = world // 2, world - 1
    steps = []
    # 1. uneven n_local (rank % 3), one of the tables empty
    uneven = []
    for i in range(rank % 3):
        k = EMPTY if i == 1 else draw(rng, D, 1500 + 100 * rank)
        uneven.append((k, counts(rng, k)))
    steps.append(("1-uneven", uneven, {}))
    # 2. nobody brings anything
    steps.append(("2-nothing", [], {}))
    # 3. the middle rank brings MAX_LOCAL tiny samples, the others one small one each
    tiny = []
    for i in range(MAX_LOCAL if rank == mid else 1):
        k = draw(rng, D, int(rng.integers(5, 41)) if rank == mid else int(rng.integers(30, 61)), must=False, edges=False)
        tiny.append((k, counts(rng, k)))
    assert len(tiny) <= MAX_LOCAL
    steps.append(("3-max-local", tiny, {}))
    # 4. every table lies inside rank 1's k-mer range: all table bytes to one rank, all hits from one rank
    lo, hi = int(bounds[1]), int(bounds[2])
    assert lo < hi
    keys = np.concatenate([D["pool"], D["edges"]]) if D["edges"] is not None else D["pool"]
    inr = keys[(keys >= np.uint64(lo)) & (keys < np.uint64(hi))]
    if len(inr) >= 50:
        k = np.sort(rng.choice(inr, size=min(len(inr), 400), replace=False))
    else:                                # (D1: no k-mer of the database lies in the range; D3: only the two edge keys do)
        k = np.unique(np.concatenate([rng.integers(lo, hi, size=200, dtype=np.uint64), inr]))
    assert len(k) and int(k[0]) >= lo and int(k[-1]) < hi
    steps.append(("4-one-range", [(k, counts(rng, k))], {}))
    # 5. wide counts on rank 0, one-byte counts on the last rank, two-byte counts between
    k = draw(rng, D, 2000)
    top = 3_000_000_001 if rank == 0 else 256 if rank == last else 60001
    c = counts(rng, k, top)
    if rank == 0:
        c[::7] = 3_000_000_000
    steps.append(("5-counts", [(k, c)], {}))
    # 6. device-resident tables: step 1's, the empty table as a null pointer
    steps.append(("6-device", uneven, dict(device_ptrs=True)))
    # 7. the length filter looks at the WHOLE genome, whose postings lie on several ranks
    short = D["genomes"][D["short"]] if D["short"] is not None else EMPTY
    k = np.unique(np.concatenate([draw(rng, D, 1500), short]))
    filt = [(k, counts(rng, k))]
    steps.append(("7-min0", filt, dict(min_number_kmers=0.0)))
    steps.append(("7-min50", filt, dict(min_number_kmers=50.0)))
    # 8. injected host-side failure (fail_next_shard_probe), then an ordinary batch
    k = draw(rng, D, 1200)
    plain = [(k, counts(rng, k))]
    steps.append(("8-fail-mid", plain, dict(fail=(mid,))))
    steps.append(("8-fail-two", plain, dict(fail=(1, last))))
    return steps


# With 3 and 5 ranks every step runs on every database under every cut and both reduces: 180 lines, 216 exchanges, ~1 s of a ~5 s launch.
# With 8 ranks one exchange was measured at 118-127 ms in three sessions and 43 ms in a fourth instead of ~5 ms (9 processes hold the GPU
# open, pytest's own context included), and the full list made the launch 33 s: 6.5 times the two-rank test's 5 s.  The 8-rank launch
# therefore keeps every step on D0 and, on the other databases, the steps that meet what is special about them: 80 lines, 88 exchanges,
# 16 s (8.6 s in the fast session).  Each of those still runs under both reduces and every cut.
PLAN_AT_8 = {
    ("D1", "kmer"): ("1-uneven", "4-one-range", "5-counts"),       # ranks without a posting: uneven batches, a range nobody hits, widths
    ("D1", "genome"): ("1-uneven", "4-one-range", "5-counts"),
    ("D1", "kmer-hand"): ("1-uneven", "5-counts"),                 # hi == lo
    ("D2", "kmer"): ("1-uneven", "3-max-local", "5-counts"),       # ranks without a genome, 64 samples whose hits come from three ranks
    ("D2", "genome"): ("1-uneven", "3-max-local", "5-counts"),
    ("D3", "kmer"): ("1-uneven", "4-one-range", "5-counts"),       # the edge keys among many, and alone in rank 1's range
    ("D3", "genome"): ("1-uneven", "4-one-range", "5-counts"),
}


def planned(world, name, cut, label):
    return world < 8 or name == "D0" or label in PLAN_AT_8[(name, cut)]


def expect(D, full, goff, samples, mnk):
    """oracle.contain over the whole database per sample -> [(contain_count[G], cov_off[G + 1], every sorted vector, concatenated)]"""
    out = []
    G = len(goff) - 1
    for k, c in samples:
        ecc, ecov, _ = O.contain(k, c, full, goff, min_number_kmers=mnk)
        vec = [np.sort(ecov[g]).astype(np.uint32) for g in range(G)]
        eoff = np.zeros(G + 1, dtype=np.int64)
        eoff[1:] = np.cumsum(ecc.astype(np.int64))
        out.append((ecc, eoff, np.concatenate(vec) if G else np.zeros(0, np.uint32)))
    return out


def run(db, comm, samples, dev, device_ptrs=False, min_number_kmers=50.0):
    if not device_ptrs:
        return db.contain_batch_sharded(comm, samples, min_number_kmers=min_number_kmers)
    tk = [torch.from_numpy(k.view(np.int64)).to(dev) for k, _ in samples]
    tc = [torch.from_numpy(c.view(np.int32)).to(dev) for _, c in samples]
    torch.cuda.synchronize()
    refs = [(a.data_ptr() if a.numel() else 0, b.data_ptr() if b.numel() else 0, a.numel()) for a, b in zip(tk, tc)]
    return db.contain_batch_sharded(comm, refs, min_number_kmers=min_number_kmers, device_ptrs=True)


def check(tag, out, exp, G):
    """contain_count of every genome row; every coverage vector against np.sort(ecov[g]) (equal offsets for every row + equal
    concatenation of the sorted vectors = every vector equal), whatever width came back widened to uint32."""
    cc, off, covs = out
    n = len(exp)
    assert len(cc) == n * G and len(off) == n * G + 1 and int(off[0]) == 0, (tag, len(cc), len(off))
    off = np.asarray(off).astype(np.int64)
    covs = np.asarray(covs).astype(np.uint32)
    assert len(covs) == int(off[-1]), (tag, len(covs), int(off[-1]))
    for s, (ecc, eoff, evec) in enumerate(exp):
        assert np.array_equal(cc[s * G:(s + 1) * G], ecc), (tag, s, np.flatnonzero(np.asarray(cc[s * G:(s + 1) * G]) != ecc)[:8])
        assert np.array_equal(off[s * G:(s + 1) * G + 1] - off[s * G], eoff), (tag, s, "cov_off")
        assert np.array_equal(covs[off[s * G]:off[(s + 1) * G]], evec), (tag, s, "coverage vectors")


def main():
    torch.set_num_threads(1)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert 3 <= world <= 8
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = S.Context(0)
    comm = SH.torch_callback_comm(dist, dev)
    t_ready = time.time()
    n_batch = 0                                         # batches scheduled so far: the reduce follows its parity, on every rank alike
    lines = 0
    for di, D in enumerate((d0(world), d1(world), d2(world), d0(world, extreme=True))):
        genomes, name = D["genomes"], D["name"]
        t_db, t_exp, n_calls = time.time(), 0.0, 0
        G = len(genomes)
        full = np.concatenate(genomes)
        goff = np.zeros(G + 1, dtype=np.uint64)
        goff[1:] = np.cumsum([len(g) for g in genomes])
        assert G <= 80 and len(full) <= 40000, (name, G, len(full))
        # ---- this rank's shard under every cut
        bounds = S.shard_bounds(D["max_key"], world)
        assert np.array_equal(bounds, SH.shard_bounds(D["max_key"], world))
        cuts = [("kmer", bounds)] + ([("kmer-hand", D["hand"])] if "hand" in D else [])
        dbs = []
        for cut, b in cuts:
            db = S.Database(ctx, full, goff, shard=(b, world, rank))
            lo, hi = int(b[rank]), int(b[rank + 1])
            mine = (full >= np.uint64(lo)) & ((full < np.uint64(hi)) if rank + 1 < world else True)          # the last range is open-ended
            assert db.n_kmers == int(mine.sum()), (name, cut, rank, db.n_kmers, int(mine.sum()))
            dbs.append((cut, db))
        gb = SH.genome_shard_bounds(goff, world)
        per = [int(goff[int(gb[r + 1])] - goff[int(gb[r])]) for r in range(world)]
        db = S.Database(ctx, full, goff, genome_shard=(gb, world, rank))
        assert db.n_kmers == per[rank] and sum(per) == len(full), (name, rank, db.n_kmers, per)
        dbs.append(("genome", db))
        if name == "D0":
            g9 = genomes[D["short"]]
            assert len(g9) == 49 and len(set(np.searchsorted(bounds[1:world], g9, side="right").tolist())) >= 2   # its postings lie on several ranks
        if name == "D1":
            assert (dbs[0][1].n_kmers > 0) == (rank in (0, world - 1)), (rank, dbs[0][1].n_kmers)    # equal widths: the middle ranges hold no posting
            assert int(D["hand"][1]) == int(D["hand"][2]) and (rank != 1 or dbs[1][1].n_kmers == 0)   # hi == lo on rank 1: no index is built
        if name == "D2" and world >= 5:
            assert min(per) == 0, per                                                    # some rank holds no genome, or only empty ones
        t_up = time.time()
        # ---- the steps
        for label, samples, opt in make_steps(D, di, bounds, rank, world):
            mnk = opt.get("min_number_kmers", 50.0)
            t = time.time()
            exp = expect(D, full, goff, samples, mnk)                                   # once per step: shared by every cut and reduce
            t_exp += time.time() - t
            if name in ("D0", "D3") and label in ("1-uneven", "5-counts"):
                assert all(len(k) == 0 or int(e[0].sum()) > 4096 for (k, _), e in zip(samples, exp))     # several scatter tiles per sample
            if name in ("D0", "D3") and label.startswith("7-"):
                assert (int(exp[0][0][D["short"]]) > 0) == (mnk == 0.0)
            if name == "D3" and label in ("5-counts", "7-min50", "8-fail-mid"):
                assert int(exp[0][0][30]) >= 2 and int(exp[0][0][31]) >= len(D["edges"])  # the oracle counts 0, 2^64 - 1 and every edge key
            for _ in REDUCES:
                reduce = REDUCES[n_batch % 2]
                n_batch += 1
                ctx.set_option("shard_reduce", reduce)
                for cut, db in dbs:
                    if not planned(world, name, cut, label):
                        continue
                    tag = (name, cut, reduce, label, rank)
                    if "fail" in opt:
                        if rank in opt["fail"]:
                            ctx.set_option("fail_next_shard_probe", "1")
                        first = min(opt["fail"])                                         # plan_hits reports the first rank that failed
                        try:
                            run(db, comm, samples, dev)
                            raise AssertionError(f"{tag}: the batch with a failing rank returned normally")
                        except S.SylphHipError as e:
                            if rank == first:
                                assert "failed on this rank" in str(e) and "injected failure" in str(e), (tag, str(e))
                            else:
                                assert f"failed on rank {first} (" in str(e), (tag, str(e))
                        out = run(db, comm, samples, dev)                                # the next batch is an ordinary one
                    else:
                        out = run(db, comm, samples, dev, opt.get("device_ptrs", False), mnk)
                    if label == "2-nothing":
                        assert len(out[0]) == 0 and len(out[2]) == 0 and len(out[1]) == 1, (tag, [len(x) for x in out])
                    check(tag, out, exp, G)
                    n_calls += 2 if "fail" in opt else 1
                    if rank == 0:
                        print(f"SHARD_WORLDS_STEP {name} {cut} {reduce} {label}", flush=True)
                        lines += 1
        for _, db in dbs:
            db.close()
        if rank == 0:       # where a launch's wall time goes: start-up, uploads, the oracle, the exchanges
            print(f"SHARD_WORLDS_TIME {name} upload {t_up - t_db:.2f} s, oracle {t_exp:.2f} s, {n_calls} exchanges {time.time() - t_up - t_exp:.2f} s", flush=True)
    comm.close()
    ctx.close()
    dist.barrier()
    if rank == 0:
        print(f"SHARD_WORLDS_TIME start-up {t_ready - T0:.2f} s, all {time.time() - T0:.2f} s", flush=True)
        print(f"SHARD_WORLDS_OK world={world} lines={lines}", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
