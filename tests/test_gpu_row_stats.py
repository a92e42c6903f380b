"""GPU tests of the coverage rows summarised on the device (sylph_row_summaries, sylph_amd/csrc/row_stats.hip): every field of every
candidate against tests/row_stats_ref.py's numpy restatement of contain.rs / inference.rs, from host and from device memory at the
three widths, over rows at every length around the 64-value chunk and the crafted ones of the restatement's module; the order of the
candidates, the gathered values, the reject at, one ulp above and one ulp below a row's index, and the invalid arguments."""
import ctypes as C

import numpy as np
import pytest

from sylph_amd import binding as B

from . import row_stats_ref as RS

pytestmark = pytest.mark.gpu
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32}
MIN_COUNT_CORRECT = 3.0


@pytest.fixture(scope="module")
def H():
    return RS.host_lib()


@pytest.fixture(scope="module")
def cut(H):
    return RS.cut_table(RS.host_cdf(H))                                       # from the definition, with the host's cdf


@pytest.fixture(scope="module")
def blocks(H, cut):
    """width -> one result block: the rows that fit the width, in a fixed order, an empty row (or two) between any two of them, some
    values in front of the first row (cov_off[0] != 0); with every row's expected summary, computed once"""
    cdf = RS.host_cdf(H)
    named = dict(RS.crafted_rows())
    named.update(RS.cut_rows(cut))
    expected = {name: RS.summary_of_row(row, cdf) for name, row in named.items()}
    rng = np.random.default_rng(8)
    out = {}
    for width in (1, 2, 4):
        names = [n for n, r in named.items() if RS.width_of(r) <= width]
        rows, which = [], []
        for i, n in enumerate(names):
            for _ in range(1 + i % 2):
                rows.append(np.zeros(0, dtype=np.uint64))
                which.append(None)
            rows.append(named[n])
            which.append(n)
        rows.append(np.zeros(0, dtype=np.uint64))
        which.append(None)
        lead = 37                                                              # values that belong to no row
        off = np.zeros(len(rows) + 1, dtype=np.uint64)
        off[0] = lead
        off[1:] = lead + np.cumsum([len(r) for r in rows])
        covs = np.concatenate([np.full(lead, 9, dtype=np.uint64)] + rows).astype(DTYPE[width])
        # genomes between 1x and 400x their row: some rows reach the ANI cut, most do not
        kmers = np.array([len(r) * int(rng.choice([1, 2, 3, 5, 30, 400])) for r in rows], dtype=np.uint32)
        out[width] = dict(rows=rows, which=which, off=off, covs=covs, kmers=kmers)
    assert {"sum_wraps", "w32_lo", "max_value"} <= set(out[4]["which"]) and "w16_lo" in out[2]["which"] and "w8_edge" in out[1]["which"]
    return out, expected


def run(ctx, blk, filt, mem):
    if mem == "host":
        return B.row_summaries(ctx, blk["covs"], blk["off"], blk["kmers"], filt)
    import torch
    dev = torch.from_numpy(blk["covs"].view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return B.row_summaries(ctx, dev.data_ptr(), blk["off"], blk["kmers"], filt, cov_width=blk["covs"].dtype.itemsize)


def check(blk, expected, got, want_rows):
    rows, roff, rcovs = got
    assert rows["row"].tolist() == want_rows                                   # ascending row order, exactly the candidates
    assert len(roff) == len(rows) + 1 and roff[0] == 0
    at = 0
    for j, r in enumerate(want_rows):
        want = expected[blk["which"][r]]
        assert {f: int(rows[j][f]) for f in RS.FIELDS[1:]} == want, (blk["which"][r], r)
        assert int(roff[j]) == at
        vals = blk["rows"][r].astype(blk["covs"].dtype)
        assert np.array_equal(rcovs[at:at + len(vals)], vals), blk["which"][r]  # the gathered values are the row
        at += len(vals)
    assert int(roff[-1]) == at == len(rcovs) and rcovs.dtype == blk["covs"].dtype


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("width", [1, 2, 4])
def test_every_nonempty_row_comes_back_without_a_cut(ctx, blocks, cut, width, mem):
    """reject_below = 0: the summaries of all rows, the empty ones left out"""
    by_width, expected = blocks
    blk = by_width[width]
    want_rows = [i for i, n in enumerate(blk["which"]) if n is not None]
    check(blk, expected, run(ctx, blk, B.row_filter(cut, reject_below=0.0, min_count_correct=MIN_COUNT_CORRECT), mem), want_rows)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("width", [1, 2, 4])
@pytest.mark.parametrize("no_adj", [False, True])
def test_candidates_are_the_rows_at_or_above_the_cut(ctx, blocks, cut, width, mem, no_adj):
    by_width, expected = blocks
    blk = by_width[width]
    reject_below = 0.95 ** 31 * (1 - 2.0 ** -30)
    want_rows, n_lambda = [], 0
    for i, n in enumerate(blk["which"]):
        if n is None:
            continue
        s = expected[n]
        index = RS.containment_index(s, int(blk["kmers"][i]), MIN_COUNT_CORRECT, no_adj)
        if not no_adj and RS.lambda_of(s, MIN_COUNT_CORRECT) is not None:
            n_lambda += 1
            assert abs(index / reject_below - 1) > 1e-6                        # (the device's exp is not this interpreter's: stay off the edge)
        if not index < reject_below:
            want_rows.append(i)
    n_rows = sum(n is not None for n in blk["which"])
    assert 0 < len(want_rows) < n_rows and (no_adj or n_lambda >= 3)
    filt = B.row_filter(cut, reject_below=reject_below, min_count_correct=MIN_COUNT_CORRECT, no_adj=no_adj)
    check(blk, expected, run(ctx, blk, filt, mem), want_rows)


def test_reject_at_one_ulp_above_and_one_ulp_below_the_index(ctx, blocks, cut):
    """A row without a lambda (median above 2): its index is contain_count / row_kmers, one correctly rounded division on either side"""
    by_width, expected = blocks
    row = RS.crafted_rows()["high_median"].astype(np.uint8)
    assert expected["high_median"]["median"] > 2
    off, kmers = np.array([0, len(row)], dtype=np.uint64), np.array([1000], dtype=np.uint32)
    index = len(row) / 1000
    for reject_below, kept in ((index, True), (np.nextafter(index, 1.0), False), (np.nextafter(index, 0.0), True)):
        rows, roff, rcovs = B.row_summaries(ctx, row, off, kmers, B.row_filter(cut, reject_below=float(reject_below)))
        assert (len(rows) == 1) == kept and int(roff[-1]) == (len(row) if kept else 0) and len(rcovs) == int(roff[-1])


def test_nothing_to_summarise(ctx, cut):
    filt = B.row_filter(cut)
    for off, kmers in ((np.array([5], dtype=np.uint64), np.zeros(0, dtype=np.uint32)),
                       (np.array([5, 5, 5, 5], dtype=np.uint64), np.array([10, 0, 3], dtype=np.uint32))):
        rows, roff, rcovs = B.row_summaries(ctx, np.arange(1, 9, dtype=np.uint16), off, kmers, filt)
        assert len(rows) == 0 and roff.tolist() == [0] and len(rcovs) == 0


def test_kernel_timer_family(ctx, blocks, cut):
    by_width, _ = blocks
    ctx.profile(True)
    try:
        before = ctx.kernel_stats("row_stats")[1]
        run(ctx, by_width[1], B.row_filter(cut), "host")
        ctx.synchronize()
        assert ctx.kernel_stats("row_stats")[1] == before + 1
    finally:
        ctx.profile(False)


def test_invalid_arguments(ctx, cut):
    covs = np.array([1, 1, 2, 3], dtype=np.uint32)
    off, kmers = np.array([0, 2, 4], dtype=np.uint64), np.array([10, 10], dtype=np.uint32)
    filt = B.row_filter(cut)
    assert len(B.row_summaries(ctx, covs, off, kmers, filt)[0]) == 2

    def refused(match, *args, **kw):
        with pytest.raises(B.SylphHipError, match=match) as e:
            B.row_summaries(ctx, *args, **kw)
        assert e.value.code == -1

    import torch
    dev = torch.from_numpy(covs.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    refused("3 bytes", dev.data_ptr(), off, kmers, filt, cov_width=3)                                   # a width that is none
    refused("cov_off decreases", covs, np.array([0, 3, 2], dtype=np.uint64), kmers, filt)
    refused("row 1 has 2 values, its genome 1 k-mers", covs, off, np.array([10, 1], dtype=np.uint32), filt)
    refused("null filter", covs, off, kmers, None)
    wrong = B.row_filter(cut)
    wrong.struct_size = C.sizeof(B.RowFilter) - 8
    refused("filter of 144 bytes", covs, off, kmers, wrong)


# ---- through the pipeline ----------------------------------------------------------------------------------------------------

def pipeline_samples(ctx, seed, n):
    import sylph_amd as S
    from .sylsp_tables import pack_entries
    from .test_gpu_pipeline import small_world
    from .test_gpu_sylsp import sample_table
    rng, genomes, db_k, goff = small_world(seed)
    G = len(goff) - 1
    db = S.Database(ctx, db_k, goff)
    kinds = ["ascending", "permutation", "duplicates"]
    tables = [sample_table(rng, db_k, goff, (2 * i) % G, kinds[i % 3]) for i in range(n)]
    raws = [pack_entries(k, c) for k, c in tables]
    return db, np.diff(goff).astype(np.uint32), tables, raws


def through_pipeline(dbs, tables, raws, filt):
    """every sample through a pipeline over `dbs`, batches of up to three tables -> per sample: the result (copied) and rows_of_last()"""
    import sylph_amd as S
    p = S.Pipeline(dbs, c=50, paired=True, n_workers=2, depth=len(raws), max_batch=3)
    p.set_option("min_batch", 3)                                              # wait for full batches: a sample is not the first of its batch
    p.set_option("batch_wait_us", 3_000_000)
    if filt is not None:
        p.set_row_filter(filt)
    for i, raw in enumerate(raws):
        assert p.submit_entries(raw.ctypes.data, len(tables[i][0]), tag=i)
    out = []
    for i in range(len(raws)):
        r = p.next()
        assert r["tag"] == i
        keep = dict(n_covs=r["n_covs"], probe_batch=r["probe_batch"], replica=r["replica"], pointers=r["result_pointers"], width=r["cov_width"],
                    contain_count=r["contain_count"].copy(), cov_off=r["cov_off"].copy(), covs=np.array(r["covs"], copy=True))
        keep["rows"] = p.rows_of_last()
        out.append(keep)
    if filt is not None:
        with pytest.raises(B.SylphHipError) as e:                             # after the first submit: the wrong state
            p.set_row_filter(filt)
        assert e.value.code == -4
    p.close()
    return out


def check_filtered_against_unfiltered(ctx, glen, plain, filtered, filt):
    assert any(int(u["cov_off"][0]) != 0 for u in plain) and any(u["probe_batch"] >= 2 for u in filtered)
    n_offset = 0
    for u, f in zip(plain, filtered):
        assert all(u["pointers"]) and f["pointers"] == (0, 0, 0)              # the filtered result's three pointers are NULL
        assert f["n_covs"] == u["n_covs"] == int(u["cov_off"][-1] - u["cov_off"][0]) and f["width"] == u["width"]
        assert not u["rows"][0].size                                          # no filter: no candidates
        want_rows, want_off, want_covs = B.row_summaries(ctx, u["covs"], u["cov_off"], glen, filt)
        rows, off, covs = f["rows"]
        assert len(rows) == len(want_rows) >= 1 and rows.tolist() == want_rows.tolist()
        assert rows["row"].max() < len(glen) and (np.diff(rows["row"].astype(np.int64)) > 0).all()
        for j in range(len(rows)):
            assert np.array_equal(covs[int(off[j]):int(off[j + 1])], want_covs[int(want_off[j]):int(want_off[j + 1])]), j
        n_offset += int(off[0]) != 0
    assert n_offset >= 1                                                      # a sample behind another in its batch: its offsets do not start at 0


@pytest.mark.parametrize("reject_below", [0.0, 0.95 ** 31 * (1 - 2.0 ** -30)])
def test_pipeline_candidates_equal_the_summaries_of_the_unfiltered_result(ctx, cut, reject_below):
    db, glen, tables, raws = pipeline_samples(ctx, 47, 6)
    filt = B.row_filter(cut, reject_below=reject_below)
    plain = through_pipeline(db, tables, raws, None)
    filtered = through_pipeline(db, tables, raws, filt)
    check_filtered_against_unfiltered(ctx, glen, plain, filtered, filt)
    assert all(int((u["contain_count"] > 0).sum()) >= len(f["rows"][0]) for u, f in zip(plain, filtered))
    db.close()


def test_pipeline_candidates_over_two_replicas_sharing_the_gpu(ctx, cut):
    import sylph_amd as S
    db, glen, tables, raws = pipeline_samples(ctx, 53, 6)
    ctx2 = S.Context(0)
    reps = [db, db.replicate(ctx2)]
    filt = B.row_filter(cut, reject_below=0.95 ** 31 * (1 - 2.0 ** -30))
    plain = through_pipeline(reps, tables, raws, None)
    filtered = through_pipeline(reps, tables, raws, filt)
    assert {f["replica"] for f in filtered} == {0, 1}
    # (which samples share a batch differs between the two runs: every sample is held against its own unfiltered result)
    for u, f in zip(plain, filtered):
        assert f["pointers"] == (0, 0, 0) and f["n_covs"] == u["n_covs"]
        want_rows, want_off, want_covs = B.row_summaries(ctx, u["covs"], u["cov_off"], glen, filt)
        rows, off, covs = f["rows"]
        assert len(rows) >= 1 and rows.tolist() == want_rows.tolist()
        for j in range(len(rows)):
            assert np.array_equal(covs[int(off[j]):int(off[j + 1])], want_covs[int(want_off[j]):int(want_off[j + 1])]), j
    reps[1].close()
    ctx2.close()
    db.close()


def test_a_sharded_pipeline_refuses_the_filter_and_a_null_filter_is_refused(ctx, cut):
    import sylph_amd as S
    from .test_gpu_pipeline import small_world
    rng, genomes, db_k, goff = small_world(7)
    comm = S.Comm(0, 1, ctx=ctx, rccl_id=S.Comm.rccl_unique_id())
    db = S.Database(ctx, db_k, goff, shard=(S.shard_bounds(int(db_k.max()), 1), 1, 0))
    p = S.Pipeline(db, c=50, paired=True, n_workers=1, depth=2, max_batch=2, comm=comm)
    with pytest.raises(B.SylphHipError, match="sharded") as e:
        p.set_row_filter(B.row_filter(cut))
    assert e.value.code == -1
    p.close(); db.close(); comm.close()
    plain_db = S.Database(ctx, db_k, goff)
    p = S.Pipeline(plain_db, c=50, paired=True, n_workers=1, depth=2, max_batch=2)
    with pytest.raises(B.SylphHipError, match="null filter") as e:
        p.set_row_filter(None)
    assert e.value.code == -1
    assert p.rows_of_last()[0].size == 0                                      # nothing returned yet
    p.close(); plain_db.close()
