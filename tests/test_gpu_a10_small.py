"""GPU test of the filter dedup's two passes (csrc/a10.hip over csrc/a10_plan.h) on the smallest samples: 40 pairs plus three copies of
one pair.  At c = 20 that is fewer than 8,192 operations — ONE class range as wide as the whole key space (the slot of a word is its
residue times slot_mult), a grid that is all padding but the `split` workgroups of that range; at c = 200 a handful of occurrences, fewer
than one wavefront.  Pushed from the host (dense arrays) and from the device with borrow_until_finish (slots: a batch this small is checked
at the push, not deferred — the deferred road is test_filter_dedup_partitioned_pass_and_its_verdict's), under either pass; every table
against the filter model, the pass read from the context's counters."""
import numpy as np
import pytest

import sylph_amd as S
from oracle import oracle as O

from .helpers import concat, random_seq, revcomp
from .test_gpu_parity import assert_same_sketch

pytestmark = pytest.mark.gpu

FPR = 1e-4


@pytest.fixture(scope="module")
def sample():
    rng = np.random.default_rng(77)
    genome = random_seq(rng, 60_000)
    recs = []
    for s in rng.integers(0, len(genome) - 500, size=40):
        recs += [genome[s:s + 150], revcomp(genome[s + 200:s + 350])]
    recs += recs[10:12] * 3                                               # three copies of one pair
    b, o = concat(recs)
    model = {c: O.sketch_reads_cuckoo_model(b, o, c=c, k=31, mode=O.MODE_AVX2_COMPAT, fpr=FPR) for c in (20, 200)}
    assert model[20]["dup_removed"] > 0 and 2 * int(model[20]["counts"].sum() + model[20]["dup_removed"]) < 8192       # one class range
    assert 0 < int(model[200]["counts"].sum() + model[200]["dup_removed"]) < 64      # fewer occurrences than one wavefront has lanes
    return b, o, model


@pytest.mark.parametrize("a10,road", [("part", (1, 0)), ("walk", (0, 0))])
@pytest.mark.parametrize("host", [True, False])
@pytest.mark.parametrize("c", [20, 200])
def test_smallest_paired_samples_under_either_pass(ctx, sample, c, host, a10, road):
    import torch
    b, o, model = sample
    sk = S.ReadSketcher(ctx, c=c, k=31, paired=True, dedup_fpr=FPR, a10=a10)
    ctx.profile(True)
    try:
        if host:
            sk.push(b, o)
        else:
            sk.set_option("borrow_until_finish", 1)
            tb = torch.from_numpy(np.concatenate([b, np.zeros(64, np.uint8)])).cuda()
            to = torch.from_numpy(o.astype(np.int64)).cuda()
            torch.cuda.synchronize()
            sk.push_device(tb.data_ptr(), to.data_ptr(), len(o) - 1, int(o[-1]))
        g = sk.finish()
        got = tuple(int(ctx.kernel_stats(f)[1]) for f in ("a10_part", "a10_redo", "deferred"))
        print(f"a10_small c={c} host={host} a10={a10}: (a10_part, a10_redo, deferred) = {got}")
    finally:
        ctx.profile(False)
        sk.close()
    assert_same_sketch(g, model[c])
    assert got == road + (0,)                                             # (deferred = 0: the device push left the slots of a checked push)
