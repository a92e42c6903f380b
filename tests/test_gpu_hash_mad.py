"""mm_hash64_gfx950 multiplies by 265 with one v_mul_lo_u32 on the high word and one v_mad_u64_u32 (device_common.h mul_const_u64; the
multiply by 21, tried the same way, keeps its shift-add chain).  Random k-mers carry from the low product into the high word nearly
always, but never meet the corners: a low word of 0 or of all ones, a high word of all ones.  The steps of mm_hash64 are bijections,
so the k-mers that put chosen values in front of either multiply are computed here by running the steps backwards, and hashed by the
position kernel and by the read kernel."""
import numpy as np
import pytest

import sylph_amd as S
from oracle import oracle as O
from oracle import pyref as P

from .helpers import ACGT, concat, random_seq

M64 = (1 << 64) - 1
INV_FIRST, INV_265, INV_21 = pow((1 << 21) + 1, -1, 1 << 64), pow(265, -1, 1 << 64), pow(21, -1, 1 << 64)
LOW_WORDS = (0x00000000, 0xFFFFFFFF, 0xFF000000, 0x00FFFFFF)      # with a random high word
PER_KIND = 4                                                       # the kinds: four low words + the high word 0xFFFFFFFF, per multiply


def hash_steps(key):
    """mm_hash64 (seeding.rs:4-15), restated: -> (hash, the value that enters * 265, the value that enters * 21)."""
    t = ~(key * ((1 << 21) + 1)) & M64
    t ^= t >> 24
    in265 = t
    t = (t * 265) & M64
    t ^= t >> 14
    in21 = t
    t = (t * 21) & M64
    t ^= t >> 28
    return (t * ((1 << 31) + 1)) & M64, in265, in21


def undo_xor_shift(y, s):
    x = y
    for _ in range(64 // s + 1):
        x = y ^ (x >> s)
    return x


def key_with_in265(v):
    return ((~undo_xor_shift(v, 24)) & M64) * INV_FIRST & M64


def key_with_in21(v):
    return key_with_in265(undo_xor_shift(v, 14) * INV_265 & M64)


def revcomp_key(key, k=31):
    r = 0
    for j in range(k):
        r = (r << 2) | (3 - ((key >> (2 * j)) & 3))
    return r


def kmer_bases(key, k=31):
    return ACGT[[(key >> (2 * (k - 1 - j))) & 3 for j in range(k)]]


def engineered_kmers():
    """[(which multiply, wanted value, key)]: canonical 31-mers (below 2^62, not above their reverse complement) whose hash meets
    the wanted value in front of * 265 or * 21.  One draw in eight to twenty qualifies."""
    rng = np.random.default_rng(265021)
    out = []
    for which, make in ((265, key_with_in265), (21, key_with_in21)):
        kinds = [lambda w=w: (int(rng.integers(0, 1 << 32)) << 32) | w for w in LOW_WORDS] + [lambda: (0xFFFFFFFF << 32) | int(rng.integers(0, 1 << 32))]
        for kind in kinds:
            found = 0
            for _ in range(2000):
                v = kind()
                key = make(v)
                if key < (1 << 62) and key <= revcomp_key(key):
                    out.append((which, v, key))
                    found += 1
                    if found == PER_KIND:
                        break
            assert found == PER_KIND
    return out


@pytest.fixture(scope="module")
def kmers():
    return engineered_kmers()


def test_the_engineered_kmers_meet_their_intermediates(kmers):
    """CPU only: the generator's k-mers are canonical 31-mers, and under the restated mm_hash64 — held here against the oracle's
    Python one — the wanted value stands in front of the multiply it was made for."""
    rng = np.random.default_rng(1)
    for key in [0, 1, M64 >> 2] + [int(x) for x in rng.integers(0, 1 << 62, size=200)]:
        assert hash_steps(key)[0] == P.mm_hash64(key)
        assert undo_xor_shift(key ^ (key >> 24), 24) == key and undo_xor_shift(key ^ (key >> 14), 14) == key
    assert len(kmers) == 2 * (len(LOW_WORDS) + 1) * PER_KIND
    for which, kinds in ((265, 1), (21, 2)):
        seen = [hash_steps(key)[kinds] for w, _, key in kmers if w == which]
        for low in LOW_WORDS:
            assert sum(v & 0xFFFFFFFF == low for v in seen) >= 3
        assert sum(v >> 32 == 0xFFFFFFFF for v in seen) >= 3
    for which, v, key in kmers:
        h, in265, in21 = hash_steps(key)
        assert (in265 if which == 265 else in21) == v
        assert key < (1 << 62) and key <= revcomp_key(key)
        s = kmer_bases(key)
        assert P.fmh_seeds(bytes(s), 1, 31) == ([h] if h != M64 else [])          # the canonical choice included


def sequence_of(kmers, rng):
    """The engineered 31-mers joined by random spacers -> (sequence, start of every k-mer)."""
    parts, starts, n = [], [], 0
    for _, _, key in kmers:
        sp = random_seq(rng, int(rng.integers(1, 90)))
        parts += [sp, kmer_bases(key)]
        starts.append(n + len(sp))
        n += len(sp) + 31
    parts.append(random_seq(rng, 40))
    return np.concatenate(parts).astype(np.uint8), starts


@pytest.mark.gpu
def test_position_kernel_hashes_the_corners(ctx, kmers):
    """extract_markers at c = 1, scalar order: the hash of every k-mer in position order (2^64 - 1 alone can never pass h < T)."""
    rng = np.random.default_rng(31)
    seq, starts = sequence_of(kmers, rng)
    assert len(seq) <= 20000
    want = P.fmh_seeds_positions(bytes(seq), 1, 31)
    at = dict(want)
    for (_, _, key), s in zip(kmers, starts):
        assert at[s + 30] == hash_steps(key)[0]
    got = ctx.extract_markers(seq, c=1, k=31, seed_mode=S.SEED_SCALAR)
    assert got.tolist() == [h for _, h in want]
    seq21 = random_seq(rng, 5003)
    got = ctx.extract_markers(seq21, c=1, k=21, seed_mode=S.SEED_SCALAR)
    assert got.tolist() == P.fmh_seeds(bytes(seq21), 1, 21)


def sketch_once(ctx, b, off, c):
    sk = S.ReadSketcher(ctx, c=c, k=31, paired=True)
    sk.push(b, off)
    r = sk.finish()
    sk.close()
    return r


@pytest.mark.gpu
def test_read_kernel_hashes_the_corners_in_every_spelling(ctx, kmers):
    """600 pairs of 2 x 150 bp — full blocks of 256 records and a partial one — that carry the engineered k-mers at every offset of a
    read, its two ends included: the compiler's hash (reads_hash 0), the pinned one and the high-word test (1, 2) give one table, the
    CPU oracle's."""
    rng = np.random.default_rng(150)
    recs = []
    for i in range(1200):
        r = random_seq(rng, 150)
        if i % 4 != 3:
            o = (0, 119, (i // 4) % 120)[i % 4]
            r[o:o + 31] = kmer_bases(kmers[(i - i // 4) % len(kmers)][2])
        recs.append(r)
    b, off = concat(recs)
    try:
        for c in (2, 200):
            e = O.sketch_reads(b, off, c=c, k=31, paired=True)
            carried = {hash_steps(key)[0] for _, _, key in kmers if hash_steps(key)[0] < M64 // c}
            assert carried <= set(e["kmers"].tolist()) and (c != 2 or len(carried) >= 10)
            for hv in (0, 1, 2):
                ctx.set_option("reads_hash", str(hv))
                g = sketch_once(ctx, b, off, c)
                assert np.array_equal(g["kmers"], e["kmers"]), (c, hv)
                assert np.array_equal(g["counts"], e["counts"]), (c, hv)
                assert g["dup_removed"] == e["dup_removed"], (c, hv)
    finally:
        ctx.set_option("reads_hash", "-1")
