#!/usr/bin/env python3
"""One genome larger than a device batch through the genome accumulator (csrc/genome_acc.hip), at two cuts.

Builds a synthetic genome of --bases bases (default 5e9) in --contigs contigs with repeats copied between contigs that lie far apart,
sketches it through Context.genome_acc twice — pushes cut greedily below L = 2^32 - 4096 and below L = 2^30, the rule of
csrc/genome_acc_plan.h restated here — and checks that the two results are identical, and equal to the CPU oracle's sketch_genome
unless --no-oracle.  Prints for each run the wall time of the pushes and of the finish, the seeds, and the peak HBM the context held
(the context's pool keeps every block it ever took until the context goes, so the device memory in use behind the finish, less what
was in use before the context existed, is the run's peak).

    python tools/genome_acc_bench.py [--bases 5000000000] [--contigs 4000] [-c 200] [-k 31] [--no-oracle]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PUSH_LIMIT = 2**32 - 4096


def build_genome(n_bases, n_contigs, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 1.5, size=n_contigs)
    lens = np.floor(w / w.sum() * n_bases).astype(np.int64)          # between a half and three halves of the mean
    lens[-1] += n_bases - int(lens.sum())                            # (the rounding's remainder: fewer than n_contigs bases)
    assert lens.min() > 10_000 and int(lens.sum()) == n_bases
    off = np.zeros(n_contigs + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    lut = np.frombuffer(b"ACGT" * 64, dtype=np.uint8)
    bases = np.empty(n_bases, dtype=np.uint8)
    step = 1 << 28
    for a in range(0, n_bases, step):
        e = min(n_bases, a + step)
        bases[a:e] = lut[rng.integers(0, 256, size=e - a, dtype=np.uint8)]
    # repeats: 5 kb of contig i copied into the contig half a genome away, so that the copies never share a push
    n_rep = max(1, n_contigs // 8)
    for i in rng.choice(n_contigs // 2, size=n_rep, replace=False):
        j = int(i) + n_contigs // 2
        a, b = int(off[i]) + 2000, int(off[j]) + 3000
        bases[b:b + 5000] = bases[a:a + 5000]
    return bases, off


def cut(lens, limit):
    """greedy runs of whole contigs below `limit` (genome_acc_plan.h cut) -> [(first, end)]"""
    runs, first, total = [], 0, 0
    for i, n in enumerate(lens):
        assert n < limit, "a contig alone holds the limit"
        if total + n >= limit:
            runs.append((first, i))
            first, total = i, 0
        total += n
    if first < len(lens):
        runs.append((first, len(lens)))
    return runs


def used_hbm():
    import torch
    free, total = torch.cuda.mem_get_info(0)
    return total - free


def run(S, bases, off, limit, args):
    import torch
    torch.cuda.synchronize()
    before = used_hbm()
    ctx = S.Context(0)
    acc = ctx.genome_acc(c=args.c, k=args.k, min_spacing=args.min_spacing, pseudotax=True)
    lens = np.diff(off.astype(np.int64))
    runs = cut(lens.tolist(), limit)
    t0 = time.perf_counter()
    for a, e in runs:
        acc.push(bases[int(off[a]):int(off[e])], off[a:e + 1] - off[a])
    ctx.synchronize()
    t_push = time.perf_counter() - t0
    n_contigs, n_bases, n_seeds = acc.counts()
    held_pushes = used_hbm() - before
    t0 = time.perf_counter()
    out = acc.finish()
    t_finish = time.perf_counter() - t0
    peak = used_hbm() - before
    acc.close()
    ctx.close()
    print(f"L={limit}: pushes={len(runs)} contigs={n_contigs} bases={n_bases} seeds={n_seeds} "
          f"push_wall={t_push:.3f} s ({t_push / (n_bases / 1e9):.3f} s/Gbp) finish_wall={t_finish:.3f} s "
          f"kept={len(out['genome_kmers'])} tracked={len(out['tracked'])} "
          f"hbm_after_pushes={held_pushes / 2**20:.0f} MiB peak_hbm={peak / 2**20:.0f} MiB "
          f"(largest push {max(int(off[e] - off[a]) for a, e in runs) / 2**20:.0f} MiB of bases; "
          f"{(peak - held_pushes) / max(1, n_seeds):.1f} B/seed taken by the finish beyond the pushes' pool)", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=5_000_000_000)
    ap.add_argument("--contigs", type=int, default=4000)
    ap.add_argument("-c", type=int, default=200)
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("--min-spacing", type=int, default=30)
    ap.add_argument("--limits", type=str, default=f"{PUSH_LIMIT},{2**30}")
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--seed", type=int, default=20261021)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import sylph_amd as S
    t0 = time.perf_counter()
    bases, off = build_genome(args.bases, args.contigs, args.seed)
    print(f"genome: {len(bases)} bases in {len(off) - 1} contigs ({time.perf_counter() - t0:.1f} s to build), c={args.c} k={args.k} "
          f"min_spacing={args.min_spacing}", flush=True)
    outs = [run(S, bases, off, int(limit), args) for limit in args.limits.split(",")]
    for o in outs[1:]:
        assert np.array_equal(o["genome_kmers"], outs[0]["genome_kmers"]) and np.array_equal(o["tracked"], outs[0]["tracked"]), "the cuts disagree"
    print(f"results at {len(outs)} cuts identical: {len(outs[0]['genome_kmers'])} kept, {len(outs[0]['tracked'])} tracked", flush=True)
    if not args.no_oracle:
        from oracle import oracle as O
        t0 = time.perf_counter()
        try:
            e = O.sketch_genome(bases, off, c=args.c, k=args.k, min_spacing=args.min_spacing, pseudotax=True)
        except (ValueError, MemoryError) as err:
            print(f"oracle.sketch_genome does not accept {len(bases)} bases: {err}", flush=True)
        else:
            assert np.array_equal(e["genome_kmers"], outs[0]["genome_kmers"]) and np.array_equal(e["tracked"], outs[0]["tracked"]), "differs from the oracle"
            print(f"oracle.sketch_genome accepts {len(bases)} bases and agrees: {e['n_raw_seeds']} seeds, {e['n_dup_kmers']} duplicate k-mers "
                  f"({time.perf_counter() - t0:.1f} s on the CPU)", flush=True)
    print("genome_acc_bench ok", flush=True)


if __name__ == "__main__":
    main()
