"""CPU tests: the oracle against (a) SURVEY Appendix A known answers (independent numpy restatement),
(b) its own committed fixtures, (c) internal consistency (scalar vs AVX2-compat vs AVX2 intrinsics)."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O

from .helpers import a10_item_hash as _a10_item_hash, a10_reduced_key as _a10_reduced_key, concat, hist, random_seq, xor_sum


@pytest.fixture(scope="module")
def kat(golden_dir):
    with open(os.path.join(golden_dir, "survey_kat.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def full(golden_dir):
    with open(os.path.join(golden_dir, "full_genome_kat.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def reads(golden_dir):
    return np.load(os.path.join(golden_dir, "k12_reads.npz"))


@pytest.fixture(scope="module")
def slices(golden_dir):
    return np.load(os.path.join(golden_dir, "ecoli_slices.npz"))


def test_hash_known_answers(kat):
    for k, v in kat["mm_hash64"].items():
        assert O.mm_hash64(int(k)) == int(v)
    # the shipped hash is NOT the textbook variant (SURVEY A.1 trap 1)
    assert O.mm_hash64(19238239812933123) != int(kat["textbook_variant_first_key"])
    for c, t in kat["threshold"].items():
        assert O.threshold(int(c)) == int(t)


def test_byte_to_seq_table():
    lut = [O.lib().orc_byte_to_seq(b) for b in range(256)]
    expect = [0] * 256
    for ch, v in (("A", 0), ("C", 1), ("G", 2), ("T", 3), ("U", 3)):
        expect[ord(ch)] = v
        expect[ord(ch.lower())] = v
    expect[1], expect[2], expect[3] = 1, 2, 3
    assert lut == expect


def test_full_genome_sketches_match_survey(kat, full):
    for f, e in kat["genomes"].items():
        for mode in ("scalar", "avx2"):   # identical under both modes for these files
            g = full[f"{f}:{mode}"]
            assert g["contigs"] == e["contigs"] and g["gn_size"] == e["gn_size"]
            assert g["raw"] == e["raw"] and g["dup"] == e["dup"]
            assert g["genome_kmers"] == e["genome_kmers"] and g["tracked"] == e["tracked"]
            assert g["first3"] == e["first3"]


def test_read_sketches_match_survey(kat, full):
    for name, e in kat["reads"].items():
        for mode in ("scalar", "avx2"):
            s = full[f"{name}:{mode}"]
            assert s["distinct"] == e["distinct"] and s["total"] == e["total"] and s["hist"] == e["hist"]
            assert s["keys"][1] == e["keys_xor"] and s["keys"][2] == e["keys_sum"]
            if "mean_read_length" in e:
                assert s["mean_read_length"] == e["mean_read_length"]
            assert s["dup_removed"] == 0
    for name, e in kat["dedup"].items():
        s = full[f"{name}:avx2"]
        for key in ("distinct", "total", "dup_removed", "hist"):
            if key in e:
                assert s[key] == e[key], (name, key)


def test_containment_and_stats_match_survey(kat, full):
    for sname, per in kat["containment"].items():
        for f, (cc, n, h, naive) in per.items():
            r = full[f"contain:{sname}:{f}"]
            assert r["contain_count"] == cc and r["n_kmers"] == n and r["cov_hist"] == h
            assert abs(r["naive_ani"] - naive) < 1e-9
    for f in kat["genomes"]:
        assert full[f"contain:t_paired:{f}"]["contain_count"] == 0
        # single-end k12_R1: lambda LOW -> final ANI = naive ANI (< 0.9)
        r = full[f"contain:k12_single:{f}"]
        assert r["lambda_status"] == 0 and r["final_est_ani"] == r["naive_ani"]
    for f, e in kat["paired_stats"].items():
        r = full[f"contain:k12_paired:{f}"]
        assert r["lambda_status"] == 2
        assert abs(r["lam"] - e["lambda"]) < 1e-9 and abs(r["final_est_ani"] - e["ani"]) < 1e-9
        assert r["median_cov"] == e["median"] and abs(r["mean_cov_geq1"] - e["mean_cov_geq1"]) < 1e-9
        assert r["final_est_ani"] >= 0.95   # trap 13: naive ANI must not be used as a pre-filter


def test_per_read_seeds(kat, reads):
    for name in ("t1", "t2"):
        b, off = reads[name + "_bases"], reads[name + "_off"]
        for i in range(len(off) - 1):
            seq = b[int(off[i]):int(off[i + 1])]
            pos, h = O.extract_markers_positions(seq, mode=O.MODE_SCALAR)
            got = sorted(zip(pos.tolist(), h.tolist()))
            assert got == [tuple(x) for x in kat["per_read_seeds"][name][str(i + 1)]]


def test_poisson_cap_table(kat):
    for med, cap in kat["poisson_cap"].items():
        med = int(med)
        x = med
        while O.poisson_cdf(float(med), x + 1) < 0.9999999999:
            x += 1
        assert x == cap, (med, x, cap)


def test_toy_statistics(kat):
    t = kat["toy_stats"]
    full = np.concatenate([np.full(n, int(v), dtype=np.uint32) for v, n in t["full_covs"].items()])
    assert abs(O.ratio_lambda(full) - t["ratio_lambda"]) < 1e-12
    covs = full[full > 0]
    st = O.stats(covs, len(full))
    assert st.lambda_status == 2 and abs(st.lambda_ - 1.0) < 1e-12
    assert abs(st.final_est_ani - t["adjusted_ani"]) < 1e-9 and abs(st.naive_ani - t["naive_ani"]) < 1e-9


def test_ratio_lambda_edge_cases():
    assert O.ratio_lambda(np.array([1] * 30, dtype=np.uint32)) is None            # one distinct value
    assert O.ratio_lambda(np.array([1] * 20 + [2] * 4, dtype=np.uint32)) is None   # < 25 non-zero
    assert O.ratio_lambda(np.array([1] * 30 + [3] * 5, dtype=np.uint32)) is None   # mode+1 absent
    assert O.ratio_lambda(np.array([1] * 30 + [2] * 2, dtype=np.uint32)) is None   # count(mode+1) < 3
    assert O.ratio_lambda(np.array([0] * 100 + [1] * 30 + [2] * 3, dtype=np.uint32)) == pytest.approx(3 / 30 * 2)
    # tie on counts -> larger value is the mode (sort of (count,value) descending, inference.rs:228-230)
    assert O.ratio_lambda(np.array([1] * 15 + [2] * 15 + [3] * 5, dtype=np.uint32)) == pytest.approx(5 / 15 * 3)


def test_avx2_tail_drop_and_guards(slices):
    g = slices["g0_bases"]
    s = g[33:184]   # L=151 -> 121 k-mers, the last one is dropped by the 4-lane split
    ps, hs = O.extract_markers_positions(s, mode=O.MODE_SCALAR)
    pa, ha = O.extract_markers_positions(s, mode=O.MODE_AVX2_COMPAT)
    assert list(zip(ps.tolist(), hs.tolist())) == [(116, 4659887629048781), (150, 83502980970892378)]
    assert list(zip(pa.tolist(), ha.tolist())) == [(116, 4659887629048781)]
    rng = np.random.default_rng(1)
    for L in list(range(0, 70)) + [100, 151, 152, 153, 154]:
        seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=L)
        sc = O.extract_markers(seq, c=3, mode=O.MODE_SCALAR)
        av = O.extract_markers(seq, c=3, mode=O.MODE_AVX2_COMPAT)
        # AVX2 result == scalar result restricted to k-mer starts < 4*((L-k+1)/4), as a multiset
        psc, hsc = O.extract_markers_positions(seq, c=3, mode=O.MODE_SCALAR)
        nk = ((L - 31 + 1) // 4) * 4 if L >= 32 else 0
        keep = sorted(h for p, h in zip(psc.tolist(), hsc.tolist()) if p - 30 < nk)
        assert sorted(av.tolist()) == keep
        assert len(sc) == len(hsc)
        pav, _ = O.extract_markers_positions(seq, c=3, mode=O.MODE_AVX2_COMPAT)
        if L < 62:
            assert len(pav) == 0   # positions variant: nothing below 2k (avx2_seeding.rs:160)
    with pytest.raises(ValueError):
        O.extract_markers(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=100), k=25, mode=O.MODE_AVX2_COMPAT)


@pytest.mark.skipif(not O.lib().orc_has_avx2(), reason="host has no AVX2")
def test_avx2_intrinsics_equal_compat():
    rng = np.random.default_rng(7)
    alphabet = np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)
    for L in (31, 32, 35, 64, 150, 151, 1000, 10007):
        seq = rng.choice(alphabet, size=L)
        for k in (21, 31):
            a = O.extract_markers(seq, c=5, k=k, mode=O.MODE_AVX2_COMPAT)
            b = O.extract_markers(seq, c=5, k=k, mode=O.MODE_AVX2_FAST)
            assert a.tolist() == b.tolist()   # same emission order too
            pa = O.extract_markers_positions(seq, c=5, k=k, mode=O.MODE_AVX2_COMPAT)
            pb = O.extract_markers_positions(seq, c=5, k=k, mode=O.MODE_AVX2_FAST)
            assert pa[0].tolist() == pb[0].tolist() and pa[1].tolist() == pb[1].tolist()


def test_dedup_cutoff_and_order_dependence(slices):
    """MAX_DEDUP_COUNT cut-off vectors built from the K12 contig."""
    k12 = slices["g1_bases"]
    def reads_at(starts):
        return O.concat([bytes(k12[s:s + 70]) for s in starts])
    target = 41739749670497347
    b, off = reads_at([252, 247, 242, 237, 252])
    s = O.sketch_reads(b, off, mode=O.MODE_SCALAR)
    i = s["kmers"].tolist().index(target)
    assert s["counts"][i] == 5 and s["dup_removed"] == 0
    b, off = reads_at([252, 252, 247, 242, 237])
    s = O.sketch_reads(b, off, mode=O.MODE_SCALAR)
    i = s["kmers"].tolist().index(target)
    assert s["counts"][i] == 4 and s["dup_removed"] >= 1


def test_self_hit_marker_rule():
    """An occurrence whose two markers are equal is dropped whenever the k-mer was counted before
    (sketch.rs:709-722: m1 is looked up after m0 was inserted)."""
    rng = np.random.default_rng(3)
    core = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=40)
    def doubled(n, seed):   # s[2i]==s[2i+1] and periodic in halves -> f==g, r==t
        r = np.random.default_rng(seed)
        x = r.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n // 2)
        return np.repeat(x, 2)
    r1 = doubled(100, 1)
    r2 = doubled(100, 2)
    assert O.pair_kmer_single(r1)[0] == O.pair_kmer_single(r1)[2]
    b, off = O.concat([bytes(r1), bytes(r2), bytes(r1)])
    s = O.sketch_reads(b, off, c=1, mode=O.MODE_SCALAR)
    # every k-mer of r1 appears in read 1 and read 3; read 3's occurrences are duplicates.  k-mers of r2 that also
    # occur in r1 would be self-hit-dropped; just require consistency of totals here
    assert s["dup_removed"] > 0
    del core


def test_golden_fixtures_reproduce(reads, slices):
    for gi in range(3):
        b, off = slices[f"g{gi}_bases"], slices[f"g{gi}_off"]
        for mode, name in ((O.MODE_SCALAR, "scalar"), (O.MODE_AVX2_COMPAT, "avx2")):
            g = O.sketch_genome(b, off, mode=mode)
            assert np.array_equal(g["genome_kmers"], slices[f"g{gi}_{name}_kmers"])
            assert np.array_equal(g["tracked"], slices[f"g{gi}_{name}_tracked"])
    b, off = reads["r1_bases"], reads["r1_off"]
    s = O.sketch_reads(b, off, mode=O.MODE_AVX2_COMPAT)
    assert np.array_equal(s["kmers"], reads["k12_single_avx2_kmers"])
    assert np.array_equal(s["counts"], reads["k12_single_avx2_counts"])
    assert xor_sum(s["kmers"])[0] == 42090302901142153 and hist(s["counts"]) == {1: 509, 2: 3}


def test_a10_default_dedup_model_stays_close_to_the_exact_set():
    """a10 (sketch.rs:733-769): the reference's DEFAULT paired-end dedup is an approximate cuckoo filter (third-party crate, not in
    the tree); the GPU path implements the exact set (`--fpr 0`).  The oracle's model of the filter (published structure + the
    crate's documented defaults, oracle/sylph_oracle.cpp) bounds what that replacement costs: the k-mer set never differs, a false
    positive can only remove one more occurrence, and at --fpr 1e-4 fewer than 1 occurrence in 1,000 is affected
    (tools/a10_bound.py measures 1.8e-5 on the 1 Gbp bench-shaped sample: profiles/r03_a10_bound.txt)."""
    rng = np.random.default_rng(21)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8)
    comp[[65, 67, 71, 84]] = [84, 71, 67, 65]
    genome = rng.choice(acgt, size=400_000).astype(np.uint8)
    n_pairs, L = 60_000, 150
    start = rng.integers(0, len(genome) - 400, size=n_pairs)
    recs = np.empty((n_pairs, 2, L), dtype=np.uint8)
    recs[:, 0] = genome[start[:, None] + np.arange(L)[None, :]]
    recs[:, 1] = comp[genome[(start[:, None] + 349 - np.arange(L)[None, :])]]
    dup = rng.integers(0, n_pairs, size=3000)
    recs[rng.integers(0, n_pairs, size=3000)] = recs[dup]                 # exact duplicate pairs
    bases = recs.reshape(-1)
    off = np.arange(0, 2 * n_pairs + 1, dtype=np.uint64) * np.uint64(L)
    exact = O.sketch_reads(bases, off, c=50, k=31, paired=True)
    n_occ = int(exact["counts"].sum()) + exact["dup_removed"]
    assert exact["dup_removed"] > 1000                                     # 45x coverage: the marker test is busy
    for fpr, bound in ((1e-4, 1e-3), (1e-2, 5e-2)):
        approx = O.sketch_reads_cuckoo_model(bases, off, c=50, k=31, fpr=fpr, initial_capacity=200_000)   # (small capacity: the filter grows)
        assert np.array_equal(approx["kmers"], exact["kmers"])
        d = approx["counts"].astype(np.int64) - exact["counts"].astype(np.int64)
        assert (d <= 0).all()                                               # a false positive drops an occurrence, never adds one
        assert approx["dup_removed"] - exact["dup_removed"] == -int(d.sum())
        assert -int(d.sum()) <= bound * n_occ, (fpr, int(d.sum()), n_occ)


# ---- a10: the data-parallel formulation of the filter walk (sylph_amd/csrc/a10.hip), restated in numpy against the model's walk ----
def a10_contained_by_classes(km, marker, fpr, cap0):
    """contained[i] of the walk 'test item i, insert it when absent' WITHOUT walking: an item is contained iff it is not the first
    of its reduced-key class among the items that reach the current filter, or a closed filter holds its class; the item that
    opens filter j + 1 is the one with cap_j inserting items of phase j before it."""
    n = len(km)
    h = _a10_item_hash(km, marker)
    contained = np.zeros(n, dtype=bool)
    closed = []                                   # (fpr_j, cap_j, sorted reduced keys of the filter's members)
    begin, j = 0, 0
    while True:
        fpr_j, cap_j = fpr * 0.9 ** j, cap0 << j
        idx = np.arange(begin, n)
        prior = np.zeros(len(idx), dtype=bool)
        for (fq, cq, members) in closed:
            prior |= np.isin(_a10_reduced_key(h[idx], fq, cq), members)
        g = _a10_reduced_key(h[idx], fpr_j, cap_j)
        reach = np.flatnonzero(~prior)
        _, first = np.unique(g[reach], return_index=True)           # first occurrence of every class, in item order
        inserts = np.sort(reach[first])                              # positions (relative to begin) of the inserting items
        is_insert = np.zeros(len(idx), dtype=bool)
        is_insert[inserts] = True
        if len(inserts) <= cap_j:
            contained[idx] = ~is_insert
            return contained, j + 1
        cut = int(inserts[cap_j])                                    # relative position of the item that opens the next filter
        contained[idx[:cut]] = ~is_insert[:cut]
        closed.append((fpr_j, cap_j, np.unique(g[inserts[:cap_j]])))
        begin += cut
        j += 1


@pytest.mark.parametrize("fpr,cap0,n", [(1e-4, 10_000_000, 30_000), (0.05, 2500, 60_000), (0.3, 600, 20_000), (1e-3, 5000, 100_000)])
def test_a10_filter_walk_equals_first_of_reduced_key_class(fpr, cap0, n):
    rng = np.random.default_rng(int(n + cap0))
    km = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
    marker = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    rep = rng.integers(0, n, size=n // 5)                             # true repeats: a fifth of the items re-appear later
    at = rng.integers(0, n, size=n // 5)
    km[at], marker[at] = km[rep], marker[rep]
    walked, n_filters = O.cuckoo_walk(km, marker, fpr=fpr, initial_capacity=cap0)
    classes, n_phases = a10_contained_by_classes(km, marker, fpr, cap0)
    assert n_phases == n_filters
    assert np.array_equal(walked, classes), np.flatnonzero(walked != classes)[:10]
    exact = np.zeros(n, dtype=bool)                                   # what an exact set would have answered
    seen = set()
    for i, key in enumerate(zip(km.tolist(), marker.tolist())):
        exact[i] = key in seen
        seen.add(key)
    assert (walked | ~exact).all()                                    # no false negatives
    if fpr >= 0.05:
        assert (walked & ~exact).sum() > 10                           # and the false positives this test is about do occur


def test_sketch_files_equals_sketch_of_the_parsed_records(tmp_path):
    """orc_sketch_files (bench.py's cpu_baseline_from_files: zlib reader + record cutting + sketch, one thread per sample) gives the table
    sketch_reads gives for the same records — plain and gzip, single and paired, exact set and filter model."""
    import gzip
    rng = np.random.default_rng(5)
    g = random_seq(rng, 60000)
    recs = [g[s:s + int(rng.integers(40, 160))] for s in rng.integers(0, 59000, size=1500)]
    recs += recs[:50]
    def fq(rs, crlf=False):
        nl = b"\r\n" if crlf else b"\n"
        return b"".join(b"@r%d" % i + nl + r.tobytes() + nl + b"+" + nl + b"I" * len(r) + nl for i, r in enumerate(rs))
    m1, m2 = recs[0::2], recs[1::2]
    (tmp_path / "a_1.fq").write_bytes(fq(m1))
    (tmp_path / "a_2.fq").write_bytes(fq(m2, crlf=True))
    (tmp_path / "b_1.fq.gz").write_bytes(gzip.compress(fq(m1), 6))
    (tmp_path / "b_2.fq.gz").write_bytes(gzip.compress(fq(m2), 1))
    inter = [r for pair in zip(m1, m2) for r in pair]
    bases, off = concat(inter)
    want = O.sketch_reads(bases, off, c=20, paired=True)
    r = O.sketch_files([tmp_path / "a_1.fq", tmp_path / "b_1.fq.gz"], [tmp_path / "a_2.fq", tmp_path / "b_2.fq.gz"], c=20, fpr=0.0, threads=2)
    assert r["table_sizes"] == [len(want["kmers"])] * 2 and r["n_bases"] == [int(off[-1])] * 2 and min(r["seconds"]) > 0
    want_f = O.sketch_reads_cuckoo_model(bases, off, c=20)
    r = O.sketch_files([tmp_path / "b_1.fq.gz"], [tmp_path / "b_2.fq.gz"], c=20, fpr=1e-4)
    assert r["table_sizes"] == [len(want_f["kmers"])]
    b1, o1 = concat(m1)
    want_s = O.sketch_reads(b1, o1, c=20)
    r = O.sketch_files([tmp_path / "b_1.fq.gz", tmp_path / "a_1.fq"], None, c=20, threads=1)
    assert r["table_sizes"] == [len(want_s["kmers"])] * 2
    with pytest.raises(ValueError):
        O.sketch_files([tmp_path / "missing.fq"], None)
