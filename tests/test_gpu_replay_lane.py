"""The two bodies of the 256-slot replay kernel (replay_lds.hip, replay_bucket.h): buckets of up to 128 occurrences run with one occurrence per lane
(replay_bucket_lane), larger ones with two levels per lane (replay_bucket), in one launch.  Samples and bucket sizes that send every
bucket through the lane body, through both, through the general body only; a k-mer at the depth where the lane body hands its bucket
to the 512-slot configuration; the mate rules; a sample too small for composite keys.  Every table against the oracle, and the road
each bucket took from the library's counters ("replay_lane", "replay_general": buckets per body while profiling is on).

Which road a bucket takes is decided by its size, so the share of buckets a case leaves on the other body is a property of the
sample and the bucket map: `helpers.bucket_roads` recomputes the map of finish_bucketed on the CPU from the oracle's occurrence hashes, and
every case asserts its precondition there before it looks at the GPU's counters."""
import numpy as np
import pytest

import sylph_amd as S
from oracle import oracle as O

from .helpers import bucket_roads, concat, occurrence_hashes, random_seq, revcomp
from .test_gpu_parity import _sketch_gpu_once, assert_same_sketch, make_reads

pytestmark = pytest.mark.gpu

LANE_CAP, SEG_LIMIT = 128, 96      # replay_plan.h


class Roads:
    """Buckets per body of the sketches run inside the block, from the library's counters."""

    def __init__(self, ctx, target):
        self.ctx, self.target = ctx, target

    def __enter__(self):
        self.ctx.set_option("finish", "bucket")          # no silent detour through the device-wide path
        self.ctx.set_option("bucket_target", str(self.target))
        self.ctx.profile(True)
        return self

    def read(self):
        self.lane = int(self.ctx.kernel_stats("replay_lane")[1])
        self.general = int(self.ctx.kernel_stats("replay_general")[1])
        self.replay_launches = int(self.ctx.kernel_stats("replay")[1])
        return self

    def __exit__(self, *exc):
        self.ctx.profile(False)


@pytest.fixture(scope="module")
def lctx():
    """A context of this module's own: the cases change its bucket_target, and the option cannot be read back to restore it."""
    c = S.Context(0)
    yield c
    c.close()


SWEEP_C = 20
FILTER = dict(dedup_fpr=0.05, dedup_capacity=3000)
_cache = {}


def sweep_sample():
    """About 12,000 pairs of 2 x 150 from a 300 kb genome (c = 20, 12x: k-mers deeper than the single-end cut-off of 4), PCR duplicates,
    ragged mates; with its oracle tables and its occurrence hashes, computed once."""
    if "sweep" not in _cache:
        rng = np.random.default_rng(10)
        b, off = concat(make_reads(rng, random_seq(rng, 300000), 12000, 150, dup_frac=0.15, paired=True, insert=300))
        _cache["sweep"] = dict(b=b, off=off, hashes=occurrence_hashes(b, off, SWEEP_C),
                               paired=O.sketch_reads(b, off, c=SWEEP_C, paired=True), single=O.sketch_reads(b, off, c=SWEEP_C, paired=False),
                               filter=O.sketch_reads_cuckoo_model(b, off, c=SWEEP_C, fpr=FILTER["dedup_fpr"], initial_capacity=FILTER["dedup_capacity"]))
        assert _cache["sweep"]["single"]["counts"].max() > 4
    return _cache["sweep"]


SWEEP_MODES = {"pairs": ("paired", True, 1, {}), "single": ("single", False, 1, {}), "pairs_3_batches": ("paired", True, 3, {}),
               "filter": ("filter", True, 1, FILTER)}


@pytest.mark.parametrize("target", [64, 124, 256])
@pytest.mark.parametrize("mode", sorted(SWEEP_MODES))
def test_size_sweep(lctx, mode, target):
    s = sweep_sample()
    expect, paired, batches, dedup = SWEEP_MODES[mode]
    # the precondition, on the CPU: which body the documented map sends this sample's buckets to at this target
    roads = bucket_roads(s["hashes"], SWEEP_C, target)
    filled = roads["n"][roads["n"] > 0]
    cpu_lane, cpu_general = int((filled <= LANE_CAP).sum()), int((filled > LANE_CAP).sum())
    assert roads["composite"] and filled.max() <= 1024
    if target == 64:
        assert cpu_general < 0.01 * len(filled)
    elif target == 124:
        assert cpu_lane > 0.2 * len(filled) and cpu_general > 0.2 * len(filled)
    else:
        assert cpu_lane < 0.01 * len(filled)
    with Roads(lctx, target) as r:
        g = _sketch_gpu_once(lctx, s["b"], s["off"], paired, False, S.SEED_AVX2_COMPAT, SWEEP_C, 31, batches, **dedup)
        r.read()
    assert_same_sketch(g, s[expect], (mode, target))
    print(f"{mode} target {target}: {r.lane} lane + {r.general} general buckets on the GPU, {cpu_lane} + {cpu_general} by the map")
    assert r.lane + r.general > 0
    if target == 64:
        assert r.lane > 0 and r.general < 0.01 * (r.lane + r.general)
    elif target == 124:
        assert r.lane > 0 and r.general > 0
    else:
        assert r.general > 0


DEPTH_C, DEPTH_TARGET, DEPTH_SEED = 7, 16, 118


def depth_sample(depth):
    """Pairs of 100 bases: mate 1 of `depth` pairs is a window of a 400-base genome that holds one chosen sampled k-mer K (so K is exactly
    `depth` deep and no k-mer is deeper), their mates 2 come from the genome's far end; around them 2,000 ordinary pairs of another genome,
    which make the buckets small (16 occurrences on average: K's bucket stays below 128)."""
    key = ("depth", depth)
    if key not in _cache:
        rng = np.random.default_rng(DEPTH_SEED)
        g = random_seq(rng, 400)
        rest = make_reads(rng, random_seq(rng, 40000), 2000, 100, dup_frac=0.1, paired=True, insert=300, ragged=False)
        pos, hs = O.extract_markers_positions(g[:170], c=DEPTH_C)
        at = [i for i in range(len(pos)) if 99 <= int(pos[i]) <= 110 and int((hs == hs[i]).sum()) == 1]
        k_end, k_hash = int(pos[at[0]]), int(hs[at[0]])          # K = g[k_end - 30 .. k_end]
        pairs = []
        while len(pairs) < depth:                                # (the same first 95 pairs at every depth)
            s1 = int(rng.integers(k_end - 99, k_end - 30 + 1))   # a 100-base window that holds K ...
            s2 = int(rng.integers(220, 300 + 1))
            m1 = g[s1:s1 + 100].copy()
            if int((O.extract_markers(m1, c=DEPTH_C) == np.uint64(k_hash)).sum()) == 1:      # ... and yields it where it lies in the read
                pairs.append((m1, revcomp(g[s2:s2 + 100])))
        pairs += [(rest[i], rest[i + 1]) for i in range(0, len(rest), 2)]
        order = np.random.default_rng(depth).permutation(len(pairs))
        b, off = concat([m for i in order for m in pairs[i]])
        _cache[key] = dict(b=b, off=off, k_hash=k_hash, hashes=occurrence_hashes(b, off, DEPTH_C), paired=O.sketch_reads(b, off, c=DEPTH_C, paired=True))
    return _cache[key]


@pytest.mark.parametrize("depth", [95, 96, 97])
def test_depth_hand_off(lctx, depth):
    s = depth_sample(depth)
    roads = bucket_roads(s["hashes"], DEPTH_C, DEPTH_TARGET)
    kb = int(roads["bucket"][np.flatnonzero(s["hashes"] == np.uint64(s["k_hash"]))[0]])
    # the precondition: K is `depth` deep, its bucket is one for the lane body, its sub-range holds K alone — and nothing else in the
    # sample fills a sub-range to the limit
    assert int((s["hashes"] == np.uint64(s["k_hash"])).sum()) == depth
    assert roads["composite"] and depth < roads["n"][kb] <= LANE_CAP and roads["fill"][kb] == depth
    assert roads["n"].max() <= LANE_CAP and np.delete(roads["fill"], kb).max() < SEG_LIMIT
    with Roads(lctx, DEPTH_TARGET) as r:
        g = _sketch_gpu_once(lctx, s["b"], s["off"], True, False, S.SEED_AVX2_COMPAT, DEPTH_C, 31, 1)
        r.read()
    assert_same_sketch(g, s["paired"], depth)
    assert int(g["counts"].max()) <= depth
    print(f"depth {depth}: {r.lane} lane + {r.general} general buckets, {r.replay_launches} launch groups of the replay family")
    assert r.lane > 0 and r.general == 0                         # every bucket started in the lane body
    # the replay family's launch groups: the 256-slot kernel and the table close — and, only when a bucket was handed on, the 512-slot
    # configuration and a second table close
    assert r.replay_launches == (4 if depth >= SEG_LIMIT else 2)


def mate_rule_sample():
    if "mates" not in _cache:
        rng = np.random.default_rng(33)
        g = random_seq(rng, 60000)
        recs = make_reads(rng, g, 2500, 150, dup_frac=0.1, paired=True, insert=300)
        pairs = [(recs[i], recs[i + 1]) for i in range(0, len(recs), 2)]
        for _ in range(400):         # fragments shorter than a mate: both mates hold the same k-mers (mate-2 skip)
            s0, ins = int(rng.integers(0, len(g) - 200)), int(rng.integers(100, 150))
            frag = g[s0:s0 + ins]
            pairs.append((frag[:int(rng.integers(90, ins + 1))].copy(), revcomp(frag)[:int(rng.integers(90, ins + 1))].copy()))
        for _ in range(300):         # mate 2 a copy of mate 1: equal markers
            s0 = int(rng.integers(0, len(g) - 150))
            pairs.append((g[s0:s0 + 150].copy(), g[s0:s0 + 150].copy()))
        for _ in range(300):         # a mate under 33 bases: the pair carries no markers
            s0 = int(rng.integers(0, len(g) - 400))
            short = g[s0 + 200:s0 + 200 + int(rng.integers(20, 33))].copy()
            long = g[s0:s0 + 150].copy()
            pairs.append((long, short) if rng.random() < 0.5 else (short, long))
        pairs += [pairs[int(rng.integers(0, len(pairs)))] for _ in range(300)]      # and duplicates of all kinds
        order = rng.permutation(len(pairs))
        b, off = concat([m for i in order for m in pairs[i]])
        _cache["mates"] = dict(b=b, off=off, hashes=occurrence_hashes(b, off, 10), paired=O.sketch_reads(b, off, c=10, paired=True),
                               filter=O.sketch_reads_cuckoo_model(b, off, c=10, fpr=FILTER["dedup_fpr"], initial_capacity=FILTER["dedup_capacity"]))
    return _cache["mates"]


@pytest.mark.parametrize("mode", ["pairs", "filter"])
def test_mate_rules(lctx, mode):
    s = mate_rule_sample()
    roads = bucket_roads(s["hashes"], 10, 64)
    filled = roads["n"][roads["n"] > 0]
    assert roads["composite"] and int((filled > LANE_CAP).sum()) < 0.01 * len(filled)
    dedup = FILTER if mode == "filter" else {}
    with Roads(lctx, 64) as r:
        g = _sketch_gpu_once(lctx, s["b"], s["off"], True, False, S.SEED_AVX2_COMPAT, 10, 31, 1, **dedup)
        r.read()
    assert_same_sketch(g, s["filter" if mode == "filter" else "paired"], mode)
    assert s["paired"]["dup_removed"] > 0
    assert r.lane > 0 and r.general < 0.01 * (r.lane + r.general)


def test_tiny_sample_takes_the_general_body(lctx):
    rng = np.random.default_rng(3)
    b, off = concat(make_reads(rng, random_seq(rng, 3000), 300, 120, dup_frac=0.3, paired=True, insert=250))
    roads = bucket_roads(occurrence_hashes(b, off, 3), 3, 128)
    assert not roads["composite"] and int((roads["n"] <= LANE_CAP).sum()) > 0       # small buckets too: the map, not the size, keeps them off the lane body
    for paired in (True, False):
        with Roads(lctx, 128) as r:
            g = _sketch_gpu_once(lctx, b, off, paired, False, S.SEED_AVX2_COMPAT, 3, 31, 1)
            r.read()
        assert_same_sketch(g, O.sketch_reads(b, off, c=3, paired=paired), paired)
        assert r.lane == 0 and r.general > 0
