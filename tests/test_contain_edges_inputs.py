"""The inputs of tests/contain_edges.py meet the edges they claim — proved without a GPU: the oracle's containment equals the expectation
by construction for every builder, rows have exactly the listed lengths, and the line index's arithmetic (index_plan.h through
tests/index_plan_capi.cpp, as tests/test_index_plan.py loads it) puts genome ids, run lengths, hit keys and widths where the GPU tests
say they are.  The kernels' constants are read back from the sources: if one moves, the inputs have to move with it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import contain_edges as E
from .test_index_plan import geometry, load

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sylph_amd", "csrc")


@pytest.fixture(scope="module")
def L():
    return load(8)


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_constants_the_inputs_are_written_around():
    hits, index, probe, plan = source("hits_plan.h"), source("contain_index.h"), source("contain.hip"), source("index_plan.h")
    m = re.search(r"ROWS_TPB = (\d+), ROWS_PER_THREAD = (\d+), ROWS_TILE = ROWS_TPB \* ROWS_PER_THREAD;", hits)
    assert int(m.group(1)) * int(m.group(2)) == E.ROWS_TILE and int(m.group(1)) == 256        # (rows_scan_kernel's stride over the tiles)
    assert int(re.search(r"constexpr uint32_t SMALL_ROW = (\d+);", hits).group(1)) == E.SMALL_ROW
    assert int(re.search(r"constexpr uint32_t MAX_VALUE_LDS = (\d+);", hits).group(1)) == E.MAX_VALUE_LDS
    assert int(re.search(r"constexpr uint32_t REFS_INLINE = (\d+);", index).group(1)) == E.REFS_INLINE
    assert int(re.search(r"constexpr int PROBE_TPB = (\d+);", probe).group(1)) * 2 == E.PROBE_CHUNK and "ilp_env : 2;" in probe
    assert int(re.search(r"constexpr uint32_t LONG_RUN_MIN = (\d+);", plan).group(1)) == E.LONG_RUN_MIN
    assert "#define SYLPH_LINE_SLOTS 8" in plan


# ------------------------------------------------------------------------------------------------------------------- ladders
@pytest.mark.parametrize("name", sorted(E.ladder_cases()))
def test_ladder_case(L, name):
    case = E.ladder_cases()[name]()
    E.assert_oracle(case, 0.0)
    lengths = np.diff(case.goff.astype(np.int64))
    assert np.array_equal(case.expected_cc, lengths)                    # every key of every genome is hit: row length = genome length
    assert len(np.unique(case.db_kmers)) == len(case.db_kmers)
    mx = E.hit_max(case)
    if name.startswith("rows_"):
        assert lengths.tolist() == ([n for n in E.ROW_LENGTHS if n <= 4095] if name == "rows_descending_to_4095" else E.ROW_LENGTHS)
        for n in (E.SMALL_ROW - 1, E.SMALL_ROW, E.SMALL_ROW + 1, 255, 256, 257):
            assert n in lengths
        smap = dict(zip(case.sample_kmers.tolist(), case.sample_counts.tolist()))
        for g in range(len(lengths)):
            v = np.array([smap[k] for k in case.db_kmers[int(case.goff[g]):int(case.goff[g + 1])].tolist()], dtype=np.int64)
            if name == "rows_equal":
                assert (v == 7).all()
            elif name.startswith("rows_descending"):
                assert (np.diff(v) < 0).all() and (len(v) == 0 or v[-1] == 1)          # in table order: the keys ascend inside a genome
            elif name == "rows_alternating":
                assert set(v.tolist()) <= {3, 200} and (np.diff(v) != 0).all()
        assert mx == {"rows_equal": 7, "rows_descending": 20000, "rows_descending_to_4095": E.MAX_VALUE_LDS - 1, "rows_alternating": 200}.get(name, mx)
        assert mx < E.MAX_VALUE_LDS or name == "rows_descending"
    elif name == "max_outside_the_hits":
        assert mx == 200 and int(case.sample_counts.max()) == 3_000_000_000
    else:
        m = int(name.split("_")[1])
        row = E.BATCH_MAX_LENGTHS.index(65 if name.endswith("row65") else 1)
        assert mx == m and lengths[row] in (65, 1)
        assert sum(int((v == m).sum()) for v in case.expected_sorted_vectors) == (1 if m > 1 else int(lengths.sum()))
        assert case.expected_sorted_vectors[row][-1] == m
    assert L.ip_coverage_width(1, mx) == (1 if mx <= 255 else 2 if mx <= 65535 else 4)


def test_key_and_width_rules_at_their_edges(L):
    o = (C.c_int * 3)()
    L.ip_compact_key(65535, 65535, o)
    assert (o[0], o[1], o[2]) == (16, 16, 1)
    L.ip_compact_key(65535, 65536, o)
    assert (o[0], o[1], o[2]) == (16, 17, 0)
    top = (65534 << 16) | 65535                                          # row 65534 with a count of 65535: every bit of the 32-bit key
    assert top.bit_length() == 32
    assert [L.ip_coverage_width(1, m) for m in (255, 256, 65535, 65536)] == [1, 2, 2, 4]
    assert [L.ip_coverage_width(0, m) for m in (255, 256, 65535, 65536)] == [4, 4, 4, 4]


# ------------------------------------------------------------------------------------------------------------------- tiny genomes
@pytest.mark.parametrize("G", E.TINY_G)
def test_tiny_genome_case(L, G):
    for variant, top in ((0, None), (1, None), (2, None)) + (((0, 65535),) if G >= 65535 else ()):
        case = E.tiny_case(G, variant, top)
        E.assert_oracle(case, 0.0)
        assert len(case.goff) == G + 1 and np.array_equal(np.diff(case.goff.astype(np.int64)), np.arange(G) % 3 + 1)
        hit = np.flatnonzero(case.expected_cc).tolist()
        assert hit == E.tiny_hit_genomes(G, variant) and G - 1 in hit
        if variant != 1:
            assert 0 in hit and all(g in hit for g in (E.ROWS_TILE - 1, E.ROWS_TILE) if g < G)
        if top is not None:
            assert case.expected_sorted_vectors[G - 1][-1] == top == E.hit_max(case)
    gb = max(1, (G - 1).bit_length())
    db, goff, _ = E.tiny_db(G)
    g = geometry(L, G, 0, int(db.max()), len(db), 0)
    assert g["why"] == 0 and g["gb"] == gb and g["gshift"] == gb + 1
    assert gb == {1: 1, 2: 1, 1023: 10, 1024: 10, 1025: 11, 2047: 11, 2048: 11, 2049: 12, 4096: 12, 4097: 13, 65535: 16, 65536: 16}[G]


def test_many_tiles_case():
    case = E.many_tiles_case()
    G, S = E.MANY_TILES_G, E.MANY_TILES_S
    rows = S * G
    assert rows == 524_352 and -(-rows // E.ROWS_TILE) == 257            # one tile more than rows_scan_kernel's 256 threads take in a step
    assert len(case.sample_kmers) == S and all(len(k) == E.MANY_TILES_TABLE for k in case.sample_kmers)
    assert case.expected_cc[256 * E.ROWS_TILE:].sum() > 0 and case.expected_cc[256 * E.ROWS_TILE - 1] > 0 and case.expected_cc[0] > 0
    tiles_hit = np.unique(np.flatnonzero(case.expected_cc) // E.ROWS_TILE)
    assert len(tiles_hit) == 257                                         # every tile's total is non-zero
    E.assert_oracle(case, 0.0)


# ------------------------------------------------------------------------------------------------------------------- shared keys
def model_descriptor(L, db, goff, G, key):
    """the model index of the database -> (stored run length of the descriptor in `key`'s bucket, postings of that bucket, gb,
    what the lookup of `key` returns, whether the scan hands the run to the wavefront)"""
    gids = np.repeat(np.arange(G, dtype=np.uint32), np.diff(goff.astype(np.int64)))
    order = np.lexsort((gids, db))
    keys, gids = np.ascontiguousarray(db[order]), np.ascontiguousarray(gids[order])
    h = L.ip_model_build(keys.ctypes.data, gids.ctypes.data, len(keys), G, 0, 0, 0, 1 << 30)
    assert h
    info = np.zeros(5, dtype=np.uint64)
    L.ip_model_info(h, info.ctypes.data)
    n_buckets, div, gshift = int(info[0]), int(info[3]), int(info[4])
    lines = np.ctypeslib.as_array(L.ip_model_lines(h), shape=(n_buckets, L.SLOTS))
    b = key // div
    in_bucket = int((keys // np.uint64(div) == np.uint64(b)).sum())
    dec = np.zeros(5, dtype=np.uint64)
    L.ip_decode(int(lines[b][L.SLOTS - 1]), gshift, dec.ctypes.data)
    buf = np.zeros(len(keys) + 1, dtype=np.uint32)
    flag = C.c_int(0)
    n = L.ip_model_lookup(h, key, buf.ctypes.data, len(buf), C.byref(flag))
    got = buf[:n].tolist()
    L.ip_model_free(h)
    assert int(dec[1]) == 1
    return int(dec[4]), in_bucket, gshift - 1, got, flag.value


@pytest.mark.parametrize("G", E.SHARED_G)
def test_shared_key_case(L, G):
    for r in (1, 3):
        for short in (False, True):
            d = E.shared_key_db(G, r, short)
            assert d.holders[G - 1] and not d.short[G - 1]
            assert any(d.short) == (short and G > 1) and all(len(km) < 5 for km, s in zip(d.genomes, d.short) if s)
            for min_kmers in (0.0, 5.0):
                case = E.shared_key_case(G, r, short, min_kmers)
                E.assert_oracle(case, min_kmers)
                for g in range(G):
                    gone = d.short[g] and min_kmers == 5.0
                    assert case.expected_cc[g] == (0 if gone else r + (E.NEIGHBOURS if d.holders[g] else 0) + (1 if d.short[g] else 3))
                    assert gone or int((case.expected_sorted_vectors[g] == E.SHARED_COUNT).sum()) >= r
            # the index: the shared key and its 40 neighbours in ONE bucket, behind a descriptor whose length field saturates at 2^gb - 1
            case = E.shared_key_case(G, r, short)
            stored, in_bucket, gb, got, long_run = model_descriptor(L, case.db_kmers, case.goff, G, d.shared)
            assert gb == max(1, (G - 1).bit_length()) == geometry(L, G, 0, int(case.db_kmers.max()), len(case.db_kmers), 0)["gb"]
            assert in_bucket >= G * r + E.NEIGHBOURS * sum(d.holders)
            run = in_bucket - (L.SLOTS - 1)
            assert stored == min(run, 2**gb - 1)
            assert got == [g for g in range(G) for _ in range(r)]          # genome G - 1 = the largest id, beside the descriptor flag
            if G <= 32 and run > E.LONG_RUN_MIN:
                assert stored < E.LONG_RUN_MIN and not long_run            # saturated below LONG_RUN_MIN: one lane walks a long run
            if G >= 33:
                assert run > 63 and stored >= E.LONG_RUN_MIN and long_run  # (G 33 .. 64: saturated at 63, still long)
            if G in (5, 32):
                assert run > E.LONG_RUN_MIN                                # the G <= 32 claim is not vacuous


def test_shared_key_tied_reassignment_by_construction():
    """the by-construction expectation of the tied reassignment equals the dictionary restatement the GPU tests use (assert_reassigned)"""
    from .test_gpu_parity import assert_reassigned
    rng = np.random.default_rng(5)
    for G in (1, 2, 33, 64, 65):
        d = E.shared_key_db(G, 3)
        passing = rng.permutation(G)
        vectors, lost = E.shared_key_tied_reassignment(d, passing)
        cc = np.array([len(v) for v in vectors], dtype=np.uint32)
        off = np.concatenate([[0], np.cumsum(cc)]).astype(np.uint64)
        covs = np.concatenate(vectors)
        smap = dict(zip(d.sample_kmers.tolist(), d.sample_counts.tolist()))
        assert_reassigned((cc, off, covs, lost), d.genomes, [np.zeros(0, dtype=np.uint64)] * G, smap, passing, np.full(G, 0.97))
        assert int(lost.sum()) == 3 * (G - 1) + E.NEIGHBOURS * (sum(d.holders) - 1)


def test_shared_core_db_puts_the_cap_among_the_kept_hits():
    for cap in (255, 256, 4095, 4096, 65536, 3_000_000_000):
        genomes, tracked, sk, sc = E.shared_core_db(cap)
        assert len(genomes) == 60 and int(sc.max()) == cap and any(len(t) for t in tracked)
        smap = dict(zip(sk.tolist(), sc.tolist()))
        first_own = [int(g[-20]) for g in genomes]                        # a key only genome g holds, in no tracked set
        assert all(smap[k] == cap for k in first_own)
        others = np.concatenate([g[:-20] for g in genomes] + tracked)
        assert not np.isin(np.array(first_own, dtype=np.uint64), others).any()


# ------------------------------------------------------------------------------------------------------------------- batches
@pytest.mark.parametrize("S", E.BATCH_S)
def test_batch_case(S):
    case = E.batch_case(S)
    G = len(case.goff) - 1
    assert G == 300 and len(case.sample_kmers) == S and len(case.expected_cc) == S * G
    sizes = [len(k) for k in case.sample_kmers]
    assert sizes[0] == sizes[S // 2] == sizes[-1] == 0 and (S > E.REFS_INLINE or S == 8)
    assert {1, E.PROBE_CHUNK - 1, E.PROBE_CHUNK, E.PROBE_CHUNK + 1, 2 * E.PROBE_CHUNK + 1} <= set(sizes)
    assert (S == 8 or any(3000 <= n <= 12000 for n in sizes)) and sum(n > 2000 for n in sizes) <= 9   # (8 tables: no room beside the edges)
    assert E.hit_max(case) < 300                                          # the row path; two-byte values
    for s in range(S):
        assert (case.expected_cc[s * G:(s + 1) * G].sum() > 0) == (sizes[s] > 0), s
    E.assert_oracle(case, E.BATCH_MIN_KMERS)
    if S in (9, 64):
        wide = E.batch_case(S, "wide")
        assert E.hit_max(wide) == 70_000 and [len(k) for k in wide.sample_kmers] == sizes
        E.assert_oracle(wide, E.BATCH_MIN_KMERS)
    if S == 9:
        empty = E.batch_case(S, "empty")
        assert all(len(k) == 0 for k in empty.sample_kmers) and empty.expected_cc.sum() == 0 and len(empty.expected_cc) == S * G
