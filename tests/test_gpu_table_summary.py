"""GPU tests of K15 (csrc/table_summary.hip): sylph_table_summary and sylph_pipeline_summary_of_last against the plain walk restated in
tests/table_summary_ref.py, every field for integer equality — at the smallest shapes at which a pass can go wrong, with the test
knobs at caps 4,16 and chunk 8, on the declines, and on three seeded families of 400,000 entries at the default ladder."""
import numpy as np
import pytest

import sylph_amd as S
from oracle import oracle as O
from sylph_amd import binding
from sylph_amd.binding import MEM_DEVICE, MEM_HOST

from . import table_summary_ref as T
from .sylsp_tables import model_table, pack_entries
from .test_gpu_pipeline import sample_reads, small_world
from .test_gpu_sylsp import sample_table

pytestmark = pytest.mark.gpu
DECLINED_LADDER = T.DECLINED | T.DECLINED_LADDER
SUMS = ("total_counts", "steps", "num_1s", "num_not1s")


def answered(got, counts, rung=None):
    want = T.walk(counts)
    assert got["flags"] == 0 and {f: got[f] for f in T.WALK_FIELDS} == want, (got, want)
    if rung is not None:
        assert got["rung"] == rung, got
    return got


@pytest.fixture()
def tiny(ctx):
    """the knobs at caps 4,16 and chunk 8; the defaults again afterwards"""
    ctx.set_option("table_summary_caps", "4,16")
    ctx.set_option("table_summary_chunk", "8")
    yield ctx
    ctx.set_option("table_summary_caps", "")
    ctx.set_option("table_summary_chunk", "")
    ctx.set_option("table_summary_max_open", "64")


@pytest.fixture(scope="module")
def families():
    """(name -> counts, the walk's integers): made once, nobody writes to them"""
    out = {}
    for name, seed, depth, ones in T.FAMILIES:
        c = T.family(seed, depth, ones=ones)
        c.setflags(write=False)
        out[name] = (c, T.walk(c))
    return out


def test_smallest_tables_at_the_default_ladder(ctx):
    assert ctx.table_summary(np.zeros(0, dtype=np.uint32)) == dict.fromkeys(binding.TABLE_SUMMARY.names, 0)
    for counts in ([1], [0], [7], [2, 2], [1, 9], [2**32 - 1, 2**32 - 1], [2**31, 2**31]):
        answered(ctx.table_summary(np.array(counts, dtype=np.uint32)), counts, rung=0)
    s = ctx.table_summary(np.array([2**31, 2**31], dtype=np.uint32))
    assert s["num_not1s"] == 0 and s["total_counts"] == 2**32 and s["median_sum"] == 3        # the u32 wraps, the u64 does not
    ones = np.ones(5000, dtype=np.uint32)                                    # no step anywhere: nothing is open, nothing declines
    s = answered(ctx.table_summary(ones), ones, rung=0)
    assert s["steps"] == 0 and s["num_1s"] == 5000 and s["open_chunks"] == 0


@pytest.mark.parametrize("n", [4095, 4096, 4097, 3 * 4096, 64 * 4096 + 5])
def test_chunk_boundaries_at_the_default_ladder(ctx, n):
    """exactly one chunk, one entry less and more, three chunks with an odd number of steps in the first (the parity the later chunks
    start from), and one chunk more than a workgroup holds"""
    rng = np.random.default_rng(n)
    c = rng.poisson(6.0, size=n).astype(np.uint32) + 1
    c[:4096][c[:4096] < 2] = 2
    c[0] = 1                                                                 # 4095 steps in the first chunk
    if n >= 3 * 4096:
        c[4096 + 100:2 * 4096 - 100] = 1                                     # a stretch without a step in the middle
    s = answered(ctx.table_summary(c), c, rung=0)
    assert n < 4096 or T.walk(c[:4096])["steps"] % 2 == 1
    assert s["open_chunks"] <= (0 if n <= 4096 else 1)                       # (a last chunk of a few entries cannot close)


def test_tiny_knobs_open_chunks_second_rung_and_max_open(tiny):
    ctx = tiny
    rng = np.random.default_rng(3)
    # a chunk of eight 3s closes at cap 4; 2, 10^6, 2, 10^6 .. leaves every chunk open (the lower walk goes 1, 2, 1, 2, the upper
    # 3, 4, 3, 4), and pass 2 walks them again
    threes = np.full(64, 3, dtype=np.uint32)
    assert answered(ctx.table_summary(threes), threes, rung=0)["open_chunks"] == 0
    open16 = np.tile(np.array([2, 10**6], dtype=np.uint32), 64)              # 16 chunks of 8
    s = answered(ctx.table_summary(open16), open16, rung=0)
    assert s["open_chunks"] == 16 and s["max_state"] == 2
    # chunks without a step between chunks with steps, an odd number of steps before them
    middle = np.concatenate([np.full(23, 3), np.ones(17), np.full(24, 3), np.ones(8), [3]]).astype(np.uint32)
    answered(ctx.table_summary(middle), middle, rung=0)
    # fails the first rung (the state reaches 4) and passes the second, whose open chunks (eight steps cannot bring 0 and 16
    # together) are all walked again
    sevens = rng.integers(6, 9, size=400).astype(np.uint32)
    s = answered(ctx.table_summary(sevens), sevens, rung=1)
    assert 4 <= s["max_state"] < 16 and 40 <= s["open_chunks"] <= 50
    # random shallow tables of every length around the chunk and the workgroup (64 chunks of 8 = 512 entries)
    for n in (7, 8, 9, 15, 16, 17, 511, 512, 513, 1031):
        c = rng.poisson(1.2, size=n).astype(np.uint32)
        got, want = ctx.table_summary(c), T.walk(c)
        assert {f: got[f] for f in SUMS} == {f: want[f] for f in SUMS}
        if got["flags"] == 0:
            answered(got, c)
        else:
            assert got["flags"] == DECLINED_LADDER                           # (the state reached 16, or too many chunks stayed open)
            assert want["max_state"] >= 16 or n > 64 * 8
    # max_open: exactly as many open chunks as allowed, then one fewer
    ctx.set_option("table_summary_max_open", "16")
    assert answered(ctx.table_summary(open16), open16, rung=0)["open_chunks"] == 16
    ctx.set_option("table_summary_max_open", "15")
    s = ctx.table_summary(open16)
    assert s["flags"] == DECLINED_LADDER and s["rung"] == 2 and s["median_sum"] == 0 and {f: s[f] for f in SUMS} == {f: T.walk(open16)[f] for f in SUMS}
    with pytest.raises(S.SylphHipError):
        ctx.set_option("table_summary_caps", "4,x")
    ctx.set_option("table_summary_caps", "16,4")                             # a ladder that does not ascend is refused where it is used
    with pytest.raises(S.SylphHipError):
        ctx.table_summary(open16)


def test_the_never_coalescing_table_declines_and_the_context_goes_on(tiny):
    ctx = tiny
    never = np.tile(np.array([2, 10**6], dtype=np.uint32), 2000)             # down, up, down, up: no chunk's bounds ever meet
    s = ctx.table_summary(never)
    want = T.walk(never)
    assert s["flags"] == DECLINED_LADDER and s["rung"] == 2 and s["median_sum"] == 0 and s["max_state"] == 0
    assert {f: s[f] for f in SUMS} == {f: want[f] for f in SUMS}
    other = np.random.default_rng(8).poisson(2.0, size=300).astype(np.uint32) + 1
    answered(ctx.table_summary(other), other)                                # right behind it, on the same context
    ctx.set_option("table_summary_caps", "")
    ctx.set_option("table_summary_chunk", "")
    s = ctx.table_summary(never)                                             # at the default ladder: 4000 entries are one chunk, walked again
    assert answered(s, never, rung=0)["open_chunks"] == 1
    big = np.tile(np.array([2, 10**6], dtype=np.uint32), 200_000)            # 98 open chunks are too many; the 25 of the second rung are walked again
    assert answered(ctx.table_summary(big), big, rung=1)["open_chunks"] == 25
    answered(ctx.table_summary(other), other, rung=0)


def test_an_outlier_in_a_shallow_table_answers_on_the_first_rung(ctx):
    c = np.random.default_rng(5).poisson(2.5, size=20_000).astype(np.uint32) + 1
    c[7777] = 2**32 - 1
    c[12_000:12_010] = 10**5
    s = answered(ctx.table_summary(c), c, rung=0)
    assert s["max_state"] < 20 and s["total_counts"] > 2**32


@pytest.mark.parametrize("name,rung", [("near3", 0), ("near9", 0), ("near400", 1)])
def test_seeded_families_at_the_default_ladder(ctx, families, name, rung):
    """400,000 entries, outliers of 5*10^4 .. 2*10^6 in 1 of 5,000: NO decline, every field the walk's, on the rung the CPU simulation
    of the plan gives (tests/test_table_summary_plan.py); from host and from device memory"""
    import torch
    c, want = families[name]
    got = ctx.table_summary(c)
    assert got["flags"] == 0 and got["rung"] == rung and {f: got[f] for f in T.WALK_FIELDS} == want, (got, want)
    assert got["open_chunks"] <= 2
    dev = torch.from_numpy(np.concatenate([np.zeros(4, np.uint32), c]).view(np.int32)).cuda()
    torch.cuda.synchronize()
    again = ctx.table_summary(dev.data_ptr() + 16, n=len(c))
    assert again == got
    ctx.profile(True)
    try:
        before = ctx.kernel_stats("table_summary")[1]
        ctx.table_summary(dev.data_ptr() + 16, n=len(c))
        assert ctx.kernel_stats("table_summary")[1] == before + 1
    finally:
        ctx.profile(False)


def test_refusals(ctx):
    import torch
    dev = torch.zeros(64, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    with pytest.raises(S.SylphHipError):
        ctx.table_summary(dev.data_ptr() + 2, n=8)                           # device counts off their width
    with pytest.raises(S.SylphHipError):
        ctx.table_summary(0, n=8)                                            # null counts
    s = ctx.table_summary(dev.data_ptr(), n=2**31)                           # 2^31 entries: declined before a count is read
    assert s["flags"] == T.DECLINED | T.DECLINED_SIZE and s["steps"] == 0
    assert ctx.table_summary(dev.data_ptr(), n=64)["flags"] == 0


# ---- through the pipeline ----------------------------------------------------------------------------------------------------

def run_pipeline(db, submit_all, n, summaries, **kw):
    """n samples through a pipeline -> [(result's counts or None, summary or None)] in submission order"""
    p = S.Pipeline(db, c=50, paired=True, n_workers=2, depth=max(n, 2), max_batch=4, **kw)
    if summaries:
        p.set_option("table_summary", "1")
    else:
        with pytest.raises(S.SylphHipError) as e:
            p.summary_of_last()
        assert e.value.code == -4
    submit_all(p)
    out = []
    for i in range(n):
        r = p.next()
        assert r["tag"] == i
        out.append((np.array(r["counts"]).copy() if kw.get("want_table") else None, p.summary_of_last() if summaries else None, r["replica"], r["n_table"]))
    p.close()
    return out


def test_pipeline_summaries_of_sessions_batches_and_entries(ctx):
    """summary_of_last == the walk over the want_table counts of a second pipeline over the same samples: sessions, raw batches,
    ascending entries and an unsorted table with duplicates (sorted on the device: the order is the pipeline's), an empty sample"""
    rng, genomes, db_k, goff = small_world(51)
    db = S.Database(ctx, db_k, goff)
    reads = [sample_reads(rng, genomes, [i], 600) for i in (0, 2)]
    tables = [sample_table(rng, db_k, goff, 1, "ascending"), sample_table(rng, db_k, goff, 3, "duplicates")]
    raws = [pack_entries(k, c) for k, c in tables]
    def submit_all(p):
        sk = S.ReadSketcher(ctx, c=50, paired=True)
        sk.push(*reads[0])
        assert p.submit_session(sk, tag=0)
        b, off = reads[1]
        assert p.submit_device([(b.ctypes.data, off.ctypes.data, len(off) - 1, int(off[-1]))], tag=1, mem=MEM_HOST)
        assert p.submit_entries(raws[0].ctypes.data, len(tables[0][0]), tag=2)
        assert p.submit_entries(raws[1].ctypes.data, len(tables[1][0]), tag=3)
        assert p.submit_entries(None, 0, tag=4)
    with_tables = run_pipeline(db, submit_all, 5, False, want_table=True)
    with_summaries = run_pipeline(db, submit_all, 5, True)
    for i, ((counts, _, _, n_table), (_, s, _, n2)) in enumerate(zip(with_tables, with_summaries)):
        assert n_table == n2 == len(counts)
        answered(s, counts, rung=0)
        assert i == 4 or s["steps"] > 50
    assert np.array_equal(with_tables[3][0], model_table(*tables[1])[1]) and not np.array_equal(with_tables[3][0], tables[1][1][:len(with_tables[3][0])])
    assert with_summaries[4][1] == dict.fromkeys(binding.TABLE_SUMMARY.names, 0)
    for e in (O.sketch_reads(b, off, c=50, paired=True) for b, off in reads[:1]):
        assert np.array_equal(with_tables[0][0], e["counts"])
    db.close()


def test_pipeline_summaries_over_two_replicas_sharing_the_gpu(ctx):
    rng, genomes, db_k, goff = small_world(53)
    db = S.Database(ctx, db_k, goff)
    ctx2 = S.Context(0)
    reps = [db, db.replicate(ctx2)]
    tables = [sample_table(rng, db_k, goff, i % 5, kind) for i, kind in enumerate(["permutation", "ascending", "duplicates", "ascending"])]
    raws = [pack_entries(k, c) for k, c in tables]
    def submit_all(p):
        for i, raw in enumerate(raws):
            assert p.submit_entries(raw.ctypes.data, len(tables[i][0]), tag=i)
    got = run_pipeline(reps, submit_all, len(raws), True)
    assert {g[2] for g in got} == {0, 1}
    for (_, s, _, n_table), (k, c) in zip(got, tables):
        wc = model_table(k, c)[1]
        assert n_table == len(wc)
        answered(s, wc, rung=0)
    reps[1].close()
    ctx2.close()
    db.close()
