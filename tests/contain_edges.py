"""Inputs that put the road from a sample table to a result block (contain.hip probe, contain_index.h line scan and long-run walk,
hits.hip row assembly, contain.hip finish_hits_sorted) ON its thresholds, with the answer known by construction.  No GPU here:
tests/test_contain_edges_inputs.py proves on the CPU that every input meets the edge it claims, tests/test_gpu_contain_edges.py and
tests/contain_edges_worker.py run them on the device.

Every builder returns a Case: (db_kmers, goff, sample_kmers, sample_counts, expected_cc, expected_sorted_vectors).  For a batch
sample_kmers / sample_counts are lists of tables and the expectation runs over the rows s * G + g.

The constants the inputs are written around (the CPU test reads them back from the sources):
  hits.hip          ROWS_TILE = 256 x 8 = 2048 rows per tile, SMALL_ROW = 64, MAX_VALUE_LDS = 4096
  contain_index.h   REFS_INLINE = 8 tables in the kernel arguments
  contain.hip       a probe chunk = PROBE_TPB 256 x ILP 2 = 512 entries of one table
  index_plan.h      LONG_RUN_MIN = 48, compact_key (cb + rb <= 32), coverage_width (256, 65536)"""
import functools
from typing import NamedTuple

import numpy as np

from oracle import oracle as O

from .test_gpu_parity import crowded_db, flat_db

ROWS_TILE, SMALL_ROW, MAX_VALUE_LDS, REFS_INLINE, PROBE_CHUNK, LONG_RUN_MIN = 2048, 64, 4096, 8, 512, 48

ROW_LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 20000]
PATTERNS = ("equal", "descending", "descending_to_4095", "alternating", "random")
BATCH_MAXIMA = [1, 255, 256, 4095, 4096, 65535, 65536, 3_000_000_000]
TINY_G = [1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 65535, 65536]
SHARED_G = [1, 2, 3, 4, 5, 32, 33, 64, 65, 1024, 1025]
BATCH_S = [8, 9, 16, 33, 64, 65]
MANY_TILES_S, MANY_TILES_G, MANY_TILES_TABLE = 64, 8193, 300


class Case(NamedTuple):
    db_kmers: np.ndarray
    goff: np.ndarray
    sample_kmers: object          # one table, or a list of tables
    sample_counts: object
    expected_cc: np.ndarray
    expected_sorted_vectors: list


def distinct_keys(rng, n):
    """n distinct k-mer values below the c = 200 threshold, in random order"""
    thr = O.threshold(200)
    keys = np.unique(rng.integers(0, thr - 64, size=n + n // 8 + 64, dtype=np.uint64))
    assert len(keys) >= n
    rng.shuffle(keys)
    return keys[:n]


def sorted_table(keys, counts):
    """a sample table: unique keys ascending, their counts beside them"""
    keys, counts = np.asarray(keys, dtype=np.uint64), np.asarray(counts, dtype=np.uint32)
    assert len(np.unique(keys)) == len(keys) == len(counts)
    order = np.argsort(keys, kind="stable")
    return keys[order], counts[order]


def hit_max(case):
    """the largest count among the HITS: what decides the path (below / from MAX_VALUE_LDS) and the width of the packed values"""
    return max([int(v.max()) for v in case.expected_sorted_vectors if len(v)] + [0])


def dict_contain(db_kmers, goff, sk, sc, min_kmers):
    """The probe half of get_stats restated over a sorted table: a genome at least min_kmers long keeps, for each of its k-mers
    (repeats included), the sample's non-zero count.  -> (cc[G], sorted vectors)"""
    G = len(goff) - 1
    val = np.zeros(len(db_kmers), dtype=np.uint32)
    if len(sk):
        k, c = sorted_table(sk, sc)
        at = np.minimum(np.searchsorted(k, db_kmers), len(k) - 1)
        val = np.where(k[at] == db_kmers, c[at], 0).astype(np.uint32)
    vectors = []
    for g in range(G):
        a, b = int(goff[g]), int(goff[g + 1])
        v = val[a:b]
        vectors.append(np.sort(v[v > 0]) if b - a >= min_kmers else np.zeros(0, dtype=np.uint32))
    return np.array([len(v) for v in vectors], dtype=np.uint32), vectors


# ------------------------------------------------------------------------------------------------------------------- ladders
def ladder(row_counts, seed, outside_counts=()):
    """Genome g owns len(row_counts[g]) keys of its own (ascending inside the genome, so genome order is table order) and the sample
    holds every one of them with the count row_counts[g][j] >= 1 — plus keys no genome holds, with outside_counts.  Row g then has
    exactly those hits."""
    rng = np.random.default_rng(seed)
    lengths = [len(c) for c in row_counts]
    keys = distinct_keys(rng, sum(lengths) + len(outside_counts))
    blocks, at = [], 0
    for n in lengths:
        blocks.append(np.sort(keys[at:at + n]))
        at += n
    db, goff = flat_db(blocks)
    counts = [np.asarray(c, dtype=np.uint32) for c in row_counts]
    assert all(len(c) == 0 or c.min() >= 1 for c in counts)
    sk, sc = sorted_table(np.concatenate(blocks + [keys[at:]]), np.concatenate(counts + [np.asarray(outside_counts, dtype=np.uint32)]))
    return Case(db, goff, sk, sc, np.array(lengths, dtype=np.uint32), [np.sort(c) for c in counts])


def row_pattern(pattern, n, rng):
    if pattern == "equal":                                    # the wavefront ranking's tie rule, one histogram bin
        return np.full(n, 7, dtype=np.uint32)
    if pattern in ("descending", "descending_to_4095"):       # strictly descending in table order
        return np.arange(n, 0, -1, dtype=np.uint32)
    if pattern == "alternating":
        return np.where(np.arange(n) % 2 == 0, 3, 200).astype(np.uint32)
    return rng.integers(1, MAX_VALUE_LDS, size=n).astype(np.uint32)


def row_lengths_case(pattern):
    """Rows of exactly ROW_LENGTHS hits.  "descending" over all of them has a row of 20,000 distinct values (the sorted path, two-byte
    values); "descending_to_4095" stops at the 4095-hit row, whose largest value 4095 is the last one the histogram takes."""
    assert pattern in PATTERNS
    rng = np.random.default_rng(PATTERNS.index(pattern))
    lengths = [n for n in ROW_LENGTHS if n <= 4095] if pattern == "descending_to_4095" else ROW_LENGTHS
    return ladder([row_pattern(pattern, n, rng) for n in lengths], seed=500 + PATTERNS.index(pattern))


BATCH_MAX_LENGTHS = [65, 1, 64, 300, 5]


def batch_max_case(maximum, where):
    """The largest count among the hits is `maximum`, once: in the 65-hit row (a histogram row) or alone in the 1-hit row."""
    assert where in ("row65", "row1")
    rng = np.random.default_rng(600 + BATCH_MAXIMA.index(maximum))
    rows = [rng.integers(1, min(maximum, 200) + 1, size=n).astype(np.uint32) for n in BATCH_MAX_LENGTHS]
    if maximum > 1:
        for r in rows:
            r[r == maximum] = 1
    g = BATCH_MAX_LENGTHS.index(65 if where == "row65" else 1)
    rows[g][17 % len(rows[g])] = maximum
    case = ladder(rows, seed=650)
    assert hit_max(case) == maximum
    return case


def outside_max_case():
    """The sample's largest counts (3,000,000,000 and 70,000) belong to keys no genome holds: path and width follow the hits (<= 200)"""
    rng = np.random.default_rng(699)
    rows = [rng.integers(1, 201, size=n).astype(np.uint32) for n in BATCH_MAX_LENGTHS]
    rows[0][3] = 200
    return ladder(rows, seed=651, outside_counts=[3_000_000_000, 70_000, 5])


def ladder_cases():
    """name -> builder of every single-sample ladder case"""
    cases = {f"rows_{p}": functools.partial(row_lengths_case, p) for p in PATTERNS}
    for m in BATCH_MAXIMA:
        for where in ("row65", "row1"):
            cases[f"max_{m}_{where}"] = functools.partial(batch_max_case, m, where)
    cases["max_outside_the_hits"] = outside_max_case
    return cases


# ------------------------------------------------------------------------------------------------------------------- tiny genomes
@functools.lru_cache(maxsize=None)
def tiny_db(G):
    """G genomes of 1, 2, 3, 1, 2, 3 ... keys, all distinct (+ 300 keys no genome holds) -> db_kmers, goff, outside keys"""
    rng = np.random.default_rng(7000 + G)
    lens = np.arange(G) % 3 + 1
    keys = distinct_keys(rng, int(lens.sum()) + 300)
    goff = np.zeros(G + 1, dtype=np.uint64)
    goff[1:] = np.cumsum(lens)
    return keys[:int(lens.sum())], goff, keys[int(lens.sum()):]


def tiny_hit_genomes(G, variant):
    if variant == 1:
        return [G - 1]
    return sorted(g for g in {0, G - 1, 2047, 2048, G // 2} if 0 <= g < G)


def tiny_case(G, variant=0, top=None):
    """The genomes 0, G - 1, G / 2 and, where they exist, 2047 and 2048 (the last row of a tile and the first of the next) are hit
    with every key (variant 1: genome G - 1 alone; variant 2: other counts); top: the count of genome G - 1's last key.
    min_number_kmers = 0."""
    db, goff, outside = tiny_db(G)
    rng = np.random.default_rng(100 * G + variant)
    hit = tiny_hit_genomes(G, variant)
    vectors = [np.zeros(0, dtype=np.uint32)] * G
    keys, counts = [outside[:50]], [rng.integers(0, 10, size=50).astype(np.uint32)]
    for g in hit:
        a, b = int(goff[g]), int(goff[g + 1])
        c = rng.integers(1, 10, size=b - a).astype(np.uint32)
        if top is not None and g == G - 1:
            c[-1] = top
        keys.append(db[a:b])
        counts.append(c)
        vectors[g] = np.sort(c)
    sk, sc = sorted_table(np.concatenate(keys), np.concatenate(counts))
    return Case(db, goff, sk, sc, np.array([len(v) for v in vectors], dtype=np.uint32), vectors)


def stack_cases(cases):
    """single-sample cases over ONE database -> the batch case of their tables"""
    assert all(c.db_kmers is cases[0].db_kmers for c in cases)
    return Case(cases[0].db_kmers, cases[0].goff, [c.sample_kmers for c in cases], [c.sample_counts for c in cases],
                np.concatenate([c.expected_cc for c in cases]), [v for c in cases for v in c.expected_sorted_vectors])


def many_tiles_case():
    """64 tables of 300 keys over 8193 tiny genomes: 524,352 rows in 257 tiles of 2048, one more tile than rows_scan_kernel's 256
    threads take in one step.  Every table hits the keys of ~100 genomes drawn at random; table 0 hits genome 0 and table 63 the
    genomes from 8129 on, which are the rows of tile 256."""
    G, S, n = MANY_TILES_G, MANY_TILES_S, MANY_TILES_TABLE
    db, goff, outside = tiny_db(G)
    rng = np.random.default_rng(8193)
    tables_k, tables_c, cc, vectors = [], [], np.zeros(S * G, dtype=np.uint32), [np.zeros(0, dtype=np.uint32)] * (S * G)
    for s in range(S):
        chosen = set(int(g) for g in rng.choice(G, size=100, replace=False))
        if s == 0:
            chosen.add(0)
        if s == S - 1:
            first = ROWS_TILE * 256 - (S - 1) * G             # genome 8129 of the last table is row 524,288
            chosen.update((first - 1, first, G - 2, G - 1))
        keys, counts = [], []
        for g in sorted(chosen):
            a, b = int(goff[g]), int(goff[g + 1])
            c = rng.integers(1, 201, size=b - a).astype(np.uint32)
            keys.append(db[a:b])
            counts.append(c)
            vectors[s * G + g] = np.sort(c)
            cc[s * G + g] = b - a
        fill = n - sum(len(k) for k in keys)
        assert fill >= 0
        keys.append(rng.choice(outside, size=fill, replace=False))
        counts.append(rng.integers(0, 201, size=fill).astype(np.uint32))
        k, c = sorted_table(np.concatenate(keys), np.concatenate(counts))
        tables_k.append(k)
        tables_c.append(c)
    assert cc[0] and cc[S * G - 1] and cc[:ROWS_TILE * 256].any()
    return Case(db, goff, tables_k, tables_c, cc, vectors)


# ------------------------------------------------------------------------------------------------------------------- shared keys
class SharedKey(NamedTuple):
    genomes: list                 # per genome: its k-mers (the shared key r times)
    shared: int                   # the key every genome holds; shared + 1 .. shared + 40 are held by every second genome
    holders: list                 # whether genome g holds the 40 neighbours
    short: list                   # whether genome g is shorter than 5 k-mers
    sample_kmers: np.ndarray
    sample_counts: np.ndarray


SHARED_COUNT, NEIGHBOURS = 5, 40


def shared_key_db(G, r, short=False, count_cap=9):
    """Every genome holds one shared key r times; the 40 values behind it (one bucket, many remainders) are held by every second
    genome, G - 1 among them; six keys of its own per genome.  short: every third genome (never G - 1) holds only the shared key and
    one key of its own — r + 1 < 5 k-mers — so that min_number_kmers = 5 filters inside the shared key's run.  The sample holds the
    shared key (count 5), its neighbours, three own keys per genome and keys no genome holds; counts up to count_cap."""
    assert r in (1, 3) and G >= 1
    rng = np.random.default_rng(9000 + 10 * G + r + (5 if short else 0))
    pool = distinct_keys(rng, 1 + 6 * G + 30)
    shared = int(pool[0])
    neighbours = np.uint64(shared) + np.arange(1, NEIGHBOURS + 1, dtype=np.uint64)
    assert not np.isin(neighbours, pool).any()
    genomes, holders, shorts = [], [], []
    for g in range(G):
        own = pool[1 + 6 * g:7 + 6 * g]
        is_short = short and g % 3 == 0 and g != G - 1
        holder = (G - 1 - g) % 2 == 0 and not is_short
        rep = np.full(r, shared, dtype=np.uint64)
        genomes.append(np.concatenate([own[:1], rep]) if is_short else
                       np.concatenate([own[:3], rep, neighbours if holder else neighbours[:0], own[3:]]))
        holders.append(holder)
        shorts.append(is_short)
        assert (len(genomes[g]) < 5) == is_short
    own_in_sample = np.concatenate([pool[1 + 6 * g:7 + 6 * g:2] for g in range(G)])
    keys = np.concatenate([np.array([shared], dtype=np.uint64), neighbours, own_in_sample, pool[1 + 6 * G:]])
    counts = rng.integers(1, min(count_cap, 9) + 1, size=len(keys)).astype(np.uint32)
    counts[0] = min(SHARED_COUNT, count_cap)
    counts[1] = count_cap                                     # (a neighbour: genome G - 1 holds it)
    counts[1 + NEIGHBOURS] = count_cap                        # (genome 0's first own key)
    sk, sc = sorted_table(keys, counts)
    return SharedKey(genomes, shared, holders, shorts, sk, sc)


def shared_key_case(G, r, short=False, min_kmers=0.0):
    """cc[g] by construction: r hits of the shared key + 40 for a holder of the neighbours + its own keys in the sample; nothing for a
    genome shorter than min_kmers"""
    d = shared_key_db(G, r, short)
    smap = dict(zip(d.sample_kmers.tolist(), d.sample_counts.tolist()))
    vectors = []
    for g, km in enumerate(d.genomes):
        own = [smap[k] for k in km.tolist() if k in smap and not d.shared <= k <= d.shared + NEIGHBOURS]
        v = [smap[d.shared]] * r + ([smap[d.shared + j] for j in range(1, NEIGHBOURS + 1)] if d.holders[g] else []) + own
        assert len(own) == (1 if d.short[g] else 3)
        vectors.append(np.sort(np.array(v if len(km) >= min_kmers else [], dtype=np.uint32)))
    db, goff = flat_db(d.genomes)
    return Case(db, goff, d.sample_kmers, d.sample_counts, np.array([len(v) for v in vectors], dtype=np.uint32), vectors)


def shared_key_tied_reassignment(d, passing):
    """Every genome of `passing` with the same ANI, no tracked sets: a k-mer goes to its first holder in the passing list.
    -> (kept sorted vectors, kmers_lost) per genome"""
    G = len(d.genomes)
    smap = dict(zip(d.sample_kmers.tolist(), d.sample_counts.tolist()))
    first = int(passing[0])
    first_holder = next((int(g) for g in passing if d.holders[g]), None)
    vectors, lost = [np.zeros(0, dtype=np.uint32)] * G, np.zeros(G, dtype=np.uint32)
    for g in (int(x) for x in passing):
        v = [smap[k] for k in d.genomes[g].tolist() if k in smap and not d.shared <= k <= d.shared + NEIGHBOURS]
        r = int((d.genomes[g] == np.uint64(d.shared)).sum())
        if g == first:
            v += [smap[d.shared]] * r
        else:
            lost[g] += r
        if d.holders[g]:
            if g == first_holder:
                v += [smap[d.shared + j] for j in range(1, NEIGHBOURS + 1)]
            else:
                lost[g] += NEIGHBOURS
        vectors[g] = np.sort(np.array(v, dtype=np.uint32))
    return vectors, lost


def shared_core_db(count_cap):
    """60 strains that hold (almost) the same 250 k-mers, tracked sets that can steal them, own keys — for the reassignment pass with
    counts up to count_cap: the cap itself sits on one own key of every genome (whoever passes keeps it) and on core k-mers.
    -> genomes, tracked, sample_kmers, sample_counts"""
    rng = np.random.default_rng(6000)                         # (the same keys for every cap)
    keys = distinct_keys(rng, 250 + 120 + 60 * 20 + 500)
    core, tcore, own, outside = keys[:250], keys[250:370], keys[370:1570].reshape(60, 20), keys[1570:]
    genomes = [np.concatenate([core[rng.random(250) < 0.95], own[g]]) for g in range(60)]
    tracked = [np.concatenate([tcore[rng.random(120) < 0.9], core[rng.random(250) < 0.05]]) if g % 4 else np.zeros(0, dtype=np.uint64)
               for g in range(60)]
    sk = np.concatenate([core, tcore, own[:, :8].ravel(), outside])
    sc = np.random.default_rng(count_cap % 9973).integers(0, min(count_cap, 5) + 1, size=len(sk)).astype(np.uint32)
    sc[:250:25] = count_cap
    sc[370:370 + 60 * 8:8] = count_cap                        # own[g][0] of every genome
    sk, sc = sorted_table(sk, sc)
    return genomes, tracked, sk, sc


# ------------------------------------------------------------------------------------------------------------------- batches
@functools.lru_cache(maxsize=None)
def batch_db():
    """the crowded database of test_gpu_parity (300 genomes: overflow runs, repeats, the keys 0 and 2^64 - 1) -> pool, shared, cluster, db, goff"""
    pool, shared, cluster, genomes = crowded_db(np.random.default_rng(31), n_genomes=300)
    db, goff = flat_db(genomes)
    return pool, shared, cluster, db, goff


BATCH_TABLE_SIZES = [0, 1, 511, 512, 12000, 513, 1025, 3000, 7000, 512, 1, 1025, 511, 513]   # (a probe chunk is 512 entries)
BATCH_MIN_KMERS = 50.0


def batch_tables(S, kind="mixed"):
    """S tables over batch_db(): sizes around the probe chunk and a few large ones, empty tables first, in the middle and last.
    kind "empty": only empty tables; "wide": one count of 70,000 among the hits, which sends the whole batch down the sorted path."""
    pool, shared, cluster, db, goff = batch_db()
    rng = np.random.default_rng(3100 + S)
    sizes = [BATCH_TABLE_SIZES[s % len(BATCH_TABLE_SIZES)] for s in range(S)]
    for s in range(S):
        if sizes[s] > 2000 and s >= 3 * len(BATCH_TABLE_SIZES):       # (a few large tables, not a dozen)
            sizes[s] = 513
    sizes[0] = sizes[S // 2] = sizes[S - 1] = 0
    if kind == "empty":
        sizes = [0] * S
    tables = []
    for s, n in enumerate(sizes):
        if n == 0:
            k = np.zeros(0, dtype=np.uint64)
        elif n == 1:
            k = shared[:1]                                    # held by almost every genome: one table entry, a long run of hits
        else:
            cand = np.unique(np.concatenate([rng.choice(pool, size=n, replace=False), shared[:50 + s], cluster[::2]]))
            k = np.sort(np.concatenate([shared[:8], rng.choice(cand[~np.isin(cand, shared[:8])], size=n - 8, replace=False)]))
        c = rng.integers(0, 300, size=len(k)).astype(np.uint32)
        if n == 1:
            c[:] = 9
        if kind == "wide" and n >= 8 and s == next(i for i, m in enumerate(sizes) if m >= 8):
            c[np.isin(k, shared[:8])] = 70_000
        assert len(k) == n == len(np.unique(k))
        tables.append((k, c))
    return tables


def batch_case(S, kind="mixed"):
    """expectation: the dictionary restatement of every table, min_number_kmers = 50"""
    pool, shared, cluster, db, goff = batch_db()
    tables = batch_tables(S, kind)
    per = [dict_contain(db, goff, k, c, BATCH_MIN_KMERS) for k, c in tables]
    return Case(db, goff, [k for k, _ in tables], [c for _, c in tables], np.concatenate([cc for cc, _ in per]), [v for _, vs in per for v in vs])


# ------------------------------------------------------------------------------------------------------------------- comparisons
def assert_block(cc, off, covs, case, rows=None, tag=None):
    """a result block (contain_count, cov_off, covs) against the case's expectation: every row, or the rows [rows[0], rows[1])"""
    a, b = rows if rows is not None else (0, len(case.expected_cc))
    cc, off = np.asarray(cc), np.asarray(off).astype(np.int64)
    assert len(cc) == b - a and len(off) == b - a + 1, tag
    assert np.array_equal(cc, case.expected_cc[a:b]), tag
    assert np.array_equal(off - off[0], np.concatenate([[0], np.cumsum(case.expected_cc[a:b], dtype=np.int64)])), tag
    want = np.concatenate([v for v in case.expected_sorted_vectors[a:b] if len(v)] + [np.zeros(0, dtype=np.uint32)])
    got = np.asarray(covs)[int(off[0]):int(off[-1])]
    assert np.array_equal(got.astype(np.uint32), want), tag


def assert_oracle(case, min_kmers, tables=None):
    """O.contain gives the case's expectation (every table of a batch)"""
    G = len(case.goff) - 1
    single = not isinstance(case.sample_kmers, list)
    ks = [case.sample_kmers] if single else case.sample_kmers
    cs = [case.sample_counts] if single else case.sample_counts
    for s in (range(len(ks)) if tables is None else tables):
        ecc, ecov, _ = O.contain(ks[s], cs[s], case.db_kmers, case.goff, min_number_kmers=min_kmers)
        assert np.array_equal(ecc, case.expected_cc[s * G:(s + 1) * G]), s
        for g in np.flatnonzero(ecc).tolist() if G > 4096 else range(G):
            assert np.array_equal(np.sort(ecov[g]), case.expected_sorted_vectors[s * G + g]), (s, g)


# ------------------------------------------------------------------------------------------------------------------- on the device
# (shared by tests/test_gpu_contain_edges.py and tests/contain_edges_worker.py; ctx.profile(True) must be on: the launch counts of the
# "sort" family — the library's radix sort, only finish_hits_sorted uses it between upload and result — and of "assemble" tell which
# path a call took)
def packed_dtype(mx, n_rows, sorted_path):
    """u8 up to 255, u16 up to 65535, else u32 — on the row path and for the sorted path's compact keys; a sorted batch whose largest
    count and row count do not fit 32 bits together (index_plan::compact_key) sorts 64-bit keys and reports u32"""
    if sorted_path and max(1, int(mx).bit_length()) + max(1, int(n_rows).bit_length()) > 32:
        return np.uint32
    return np.uint8 if mx <= 255 else np.uint16 if mx <= 65535 else np.uint32


def path_checked(ctx, call, n_hits, mx, forced):
    """call() with the path it must take: the row assembly for a largest hit count below MAX_VALUE_LDS, the sorted finish from there;
    forced (SYLPH_HIP_HIT_SORT set): the sorted finish for every call, the radix sort itself whenever there is a hit.  Returns COPIES:
    the views are borrowed from the database's pinned block, and a failing test's report prints its arrays after the database is gone"""
    before = ctx.kernel_stats("sort")[1], ctx.kernel_stats("assemble")[1]
    out = tuple(np.array(a) for a in call())
    sort, assemble = ctx.kernel_stats("sort")[1] - before[0], ctx.kernel_stats("assemble")[1] - before[1]
    if forced:
        assert assemble == 0 and (sort > 0) == (n_hits > 0), (sort, assemble, n_hits)
    else:
        assert (sort > 0) == (mx >= MAX_VALUE_LDS) and (sort == 0 or n_hits > 0), (sort, mx)
    return out


def check_single(ctx, db, case, min_kmers, forced=False):
    """contain, contain_view, the packed view and a one-table batch of a single-sample case on `db`: block, value type, path"""
    sk, sc = case.sample_kmers, case.sample_counts
    mx, n_hits, n_rows = hit_max(case), int(case.expected_cc.sum()), len(case.expected_cc)
    narrow = packed_dtype(mx, n_rows, forced or mx >= MAX_VALUE_LDS)
    calls = (("contain", lambda: db.contain(sk, sc, min_number_kmers=min_kmers), np.uint32),
             ("contain_view", lambda: db.contain_view(sk, sc, min_number_kmers=min_kmers), np.uint32),
             ("packed view", lambda: db.contain_view(sk, sc, min_number_kmers=min_kmers, packed=True), narrow),
             ("one-table batch", lambda: db.contain_batch([(sk, sc)], min_number_kmers=min_kmers), narrow))
    for name, call, dtype in calls:
        cc, off, covs = path_checked(ctx, call, n_hits, mx, forced)
        assert_block(cc, off, covs, case, tag=name)
        assert n_hits == 0 or covs.dtype == dtype, (name, covs.dtype, dtype)
    return narrow


def check_batch(ctx, db, case, min_kmers, forced=False, singles=True, device=True):
    """contain_batch of a batch case on `db`: the whole block, value type and path; the same tables resident on the device (null
    pointers for empty tables); every sample's slice against its single-sample contain"""
    tables = list(zip(case.sample_kmers, case.sample_counts))
    G, n_rows = len(case.goff) - 1, len(case.expected_cc)
    mx, n_hits = hit_max(case), int(case.expected_cc.sum())
    narrow = packed_dtype(mx, n_rows, forced or mx >= MAX_VALUE_LDS)
    cc, off, covs = path_checked(ctx, lambda: db.contain_batch(tables, min_number_kmers=min_kmers), n_hits, mx, forced)
    assert_block(cc, off, covs, case, tag="batch")
    assert n_hits == 0 or covs.dtype == narrow, (covs.dtype, narrow)
    if device:
        import torch
        tk = [torch.from_numpy(k.view(np.int64)).cuda() for k, _ in tables]
        tc = [torch.from_numpy(c.view(np.int32)).cuda() for _, c in tables]
        torch.cuda.synchronize()
        refs = [(a.data_ptr() if a.numel() else 0, b.data_ptr() if b.numel() else 0, a.numel()) for a, b in zip(tk, tc)]
        cc2, off2, covs2 = path_checked(ctx, lambda: db.contain_batch(refs, min_number_kmers=min_kmers, device_ptrs=True), n_hits, mx, forced)
        assert np.array_equal(cc2, cc) and np.array_equal(off2, off) and np.array_equal(covs2, covs) and covs2.dtype == covs.dtype
    if singles:
        for s, (k, c) in enumerate(tables):
            scc, soff, scovs = db.contain(k, c, min_number_kmers=min_kmers)
            a, b = int(off[s * G]), int(off[(s + 1) * G])
            assert np.array_equal(scc, cc[s * G:(s + 1) * G]) and np.array_equal(soff.astype(np.int64) + a, off[s * G:(s + 1) * G + 1].astype(np.int64)), s
            assert np.array_equal(scovs, covs[a:b].astype(np.uint32)), s
    return narrow
