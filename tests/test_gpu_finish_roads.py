"""GPU tests of the finish loop (csrc/sketch.hip sketch_finish_impl over csrc/finish_plan.h) on combinations of its three late answers
that no other test reaches: both verdicts bad on one sample, the filter dedup without the bucket path (finish = generic, c = 1), the
refusal of finish = bucket, a marker-less sample that needs occurrence records after all.  The sample shapes are those of
test_filter_dedup_partitioned_pass_and_its_verdict (6,000 pairs of 150 bases at c = 200: the smallest that still defers).  Every table
against the oracle; the road taken is read from the context's counters, whose expected values are what the library did before the
finish became a loop (profiles/finish_roads.txt): a counter that differs is a change of behaviour."""
import numpy as np
import pytest

import sylph_amd as S
from oracle import oracle as O

from .helpers import concat, random_seq, revcomp

pytestmark = pytest.mark.gpu

COUNTERS = ("deferred", "deferred_redo", "a10_part", "a10_redo", "short_reads", "position_road", "replay_overflow")
# recorded on the parent commit's library, same order as COUNTERS
EXPECTED = {
    "both_verdicts_bad": (1, 1, 2, 1, 1, 1, 1),
    "generic_device": (0, 0, 1, 0, 1, 0, 0),
    "generic_device_bad_marks": (0, 0, 1, 1, 1, 0, 0),
    "generic_host": (0, 0, 1, 0, 1, 0, 0),
    "generic_after_deferred_push": (1, 0, 1, 0, 1, 0, 0),
    "c1_pairs": (0, 0, 1, 0, 1, 0, 0),
    "bucket_refused_c1": (0, 0, 1, 0, 1, 0, 0),
    "bucket_refused_deep": (0, 0, 0, 0, 1, 0, 0),
    "needs_records": (0, 0, 0, 0, 0, 1, 1),
}
REFUSAL = "bucket finish overflowed and finish=bucket forbids the fallback"


def assert_same_sketch(g, e):
    assert np.array_equal(g["kmers"], e["kmers"]) and np.array_equal(g["counts"], e["counts"]) and g["dup_removed"] == e["dup_removed"]


@pytest.fixture(scope="module")
def samples():
    rng = np.random.default_rng(555)
    genome = random_seq(rng, 400_000)

    def pairs(n, L=150):
        recs = []
        for s in rng.integers(0, len(genome) - 500, size=n):
            recs.append(genome[s:s + L])
            recs.append(revcomp(genome[s + 200:s + 200 + L]))
        return recs
    one = None
    for s in range(0, 5000, 7):                                            # a pair whose mate 1 carries >= 3 seeds at c = 200
        if len(O.extract_markers(genome[s:s + 150], c=200, k=31)) >= 3:
            one = [genome[s:s + 150], revcomp(genome[s + 200:s + 350])]
            break
    assert one is not None
    copies = []
    for _ in range(3000):                                                  # 3,000 copies of one item: more than the partitioned pass resolves
        copies += pairs(2) + one
    long_pair = [genome[1000:1600], revcomp(genome[1200:1350])]            # a 600-base record: not a batch for the short-read kernel
    out = {"normal": pairs(6000) + pairs(50) * 3, "copies": copies, "copies_long": copies[:9000] + long_pair + copies[9000:],
           "small": pairs(1500)}
    return {k: concat(v) for k, v in out.items()}


def sketch(ctx, b, o, borrow=True, host=False, finish=None, finish_before_push=True, **kw):
    import torch
    sk = S.ReadSketcher(ctx, **kw)
    try:
        if borrow:
            sk.set_option("borrow_until_finish", 1)
        if finish and finish_before_push:
            ctx.set_option("finish", finish)
        if host:
            sk.push(b, o)
        else:
            tb = torch.from_numpy(np.concatenate([b, np.zeros(64, np.uint8)])).cuda()
            to = torch.from_numpy(o.astype(np.int64)).cuda()
            torch.cuda.synchronize()
            sk.push_device(tb.data_ptr(), to.data_ptr(), len(o) - 1, int(o[-1]))
        if finish:
            ctx.set_option("finish", finish)
        return sk.finish()
    finally:
        ctx.set_option("finish", "auto")
        sk.close()


def check_roads(ctx, name, fn):
    ctx.profile(True)
    try:
        fn()
        got = tuple(int(ctx.kernel_stats(f)[1]) for f in COUNTERS)
    finally:
        ctx.profile(False)
    print(f"finish_roads {name}: {dict(zip(COUNTERS, got))}")
    assert got == EXPECTED[name], name


def filter_model(b, o, c):
    return O.sketch_reads_cuckoo_model(b, o, c=c, mode=O.MODE_AVX2_COMPAT, fpr=1e-4)


def test_both_verdicts_bad_on_one_borrowed_batch(ctx, samples):
    """One 600-base record among the pairs (the seeding verdict) and 3,000 copies of one pair (the filter verdict): the batch is redone
    and marked again first, then the second attempt's filter verdict sends it through the walk."""
    b, o = samples["copies_long"]
    e = filter_model(b, o, 200)
    check_roads(ctx, "both_verdicts_bad", lambda: assert_same_sketch(sketch(ctx, b, o, c=200, paired=True, dedup_fpr=1e-4), e))


def test_generic_finish_settles_the_marks_without_the_bucket_path(ctx, samples):
    b, o = samples["normal"]
    e = filter_model(b, o, 200)
    for name, kw in (("generic_device", {}), ("generic_host", dict(host=True)), ("generic_after_deferred_push", dict(finish_before_push=False))):
        check_roads(ctx, name, lambda: assert_same_sketch(sketch(ctx, b, o, finish="generic", c=200, paired=True, dedup_fpr=1e-4, **kw), e))
    b, o = samples["copies"]
    e = filter_model(b, o, 200)                                            # the filter verdict read on its own, and bad
    check_roads(ctx, "generic_device_bad_marks", lambda: assert_same_sketch(sketch(ctx, b, o, finish="generic", c=200, paired=True, dedup_fpr=1e-4), e))


def test_c1_pairs_replay_device_wide_on_settled_marks(ctx, samples):
    b, o = samples["small"]
    e = filter_model(b, o, 1)
    check_roads(ctx, "c1_pairs", lambda: assert_same_sketch(sketch(ctx, b, o, c=1, paired=True, dedup_fpr=1e-4), e))


def test_bucket_only_finish_refuses_what_the_bucket_path_declines(ctx, samples):
    b, o = samples["small"]

    def refused(b, o, **kw):
        with pytest.raises(S.SylphHipError, match=REFUSAL):
            sketch(ctx, b, o, finish="bucket", **kw)
    check_roads(ctx, "bucket_refused_c1", lambda: refused(b, o, c=1, paired=True, dedup_fpr=1e-4))
    deep = concat([b[:200]] * 3000)                                        # one k-mer 3,000 deep: a bucket beyond every configuration
    check_roads(ctx, "bucket_refused_deep", lambda: refused(deep[0], deep[1], c=3))


def test_marker_less_sample_with_one_deep_kmer_needs_records_after_all(ctx):
    """Single-end reads of more than 400 bases carry no dedup marker: hashes only, counted without occurrence records — until the
    replay's tail reports a k-mer more than 1,024 deep (reads cut from a tandem repeat of period 50), which only the usual kernels'
    overflow path takes: the records are written after all and the bucket path runs a second time."""
    rng = np.random.default_rng(556)
    genome = random_seq(rng, 300_000)
    rep = np.tile(random_seq(rng, 50), 40)                                  # 2,000 bases of period 50
    recs = []
    for _ in range(200):
        L = int(rng.integers(401, 4000))
        s = int(rng.integers(0, len(genome) - L))
        recs.append(genome[s:s + L])
    for _ in range(200):
        s = int(rng.integers(0, len(rep) - 450))
        recs.insert(int(rng.integers(0, len(recs))), rep[s:s + 450])
    b, o = concat(recs)
    e = O.sketch_reads(b, o, c=20)
    assert e["counts"].max() > 1024
    check_roads(ctx, "needs_records", lambda: assert_same_sketch(sketch(ctx, b, o, borrow=False, host=True, c=20), e))
