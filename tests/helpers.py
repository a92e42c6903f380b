import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_bytes(rel):
    """The bytes of the fixture tests/golden/<rel>.  A fixture above the repository's 1 MiB limit per committed file is kept as
    <rel>.part0, <rel>.part1, ... (pieces of at most 1,000 KiB, in order) and joined here."""
    path = os.path.join(GOLDEN, rel)
    if os.path.exists(path):
        with open(path, "rb") as f:
            return f.read()
    parts = []
    while os.path.exists(f"{path}.part{len(parts)}"):
        with open(f"{path}.part{len(parts)}", "rb") as f:
            parts.append(f.read())
    if not parts:
        raise FileNotFoundError(path)
    return b"".join(parts)


def xor_sum(a):
    x = 0
    for v in np.asarray(a).tolist():
        x ^= int(v)
    return x, int(np.sum(np.asarray(a, dtype=np.uint64), dtype=np.uint64))


def hist(c):
    u, n = np.unique(np.asarray(c), return_counts=True)
    return {int(a): int(b) for a, b in zip(u, n)}


ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def random_seq(rng, n, alphabet=ACGT):
    return rng.choice(alphabet, size=n).astype(np.uint8)


def revcomp(seq):
    comp = np.zeros(256, dtype=np.uint8)
    comp[:] = ord("N")
    for a, b in zip(b"ACGTacgt", b"TGCAtgca"):
        comp[a] = b
    return comp[np.asarray(seq, dtype=np.uint8)][::-1].copy()


def concat(records):
    off = np.zeros(len(records) + 1, dtype=np.uint64)
    if records:
        off[1:] = np.cumsum([len(r) for r in records], dtype=np.uint64)
    bases = np.concatenate([np.asarray(r, dtype=np.uint8) for r in records]) if records else np.zeros(0, dtype=np.uint8)
    return bases.astype(np.uint8), off


def bgzf_compress(data, block=65280, level=6):
    """What `bgzip` writes: gzip members of <= 64 KiB, each with the 'BC' extra subfield holding its compressed size, and the
    empty end-of-file member."""
    import struct
    import zlib
    out = bytearray()
    for a in list(range(0, len(data), block)) + [None]:
        chunk = b"" if a is None else data[a:a + block]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = co.compress(chunk) + co.flush()
        bsize = 12 + 6 + len(body) + 8
        out += b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
        out += body + struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return bytes(out)


LANE_CAP, IDX_BITS = 128, 10      # replay_plan.h


def occurrence_hashes(b, off, c):
    """Every occurrence of a sampled k-mer in the reads: what the seeding kernel hands to the replay."""
    from oracle import oracle as O
    return np.concatenate([O.extract_markers(b[int(off[i]):int(off[i + 1])], c=c) for i in range(len(off) - 1)] + [np.zeros(0, np.uint64)])


def bucket_roads(hashes, c, target):
    """The bucket map of finish_bucketed (make_bucket_map, replay_plan.h; tests/test_replay_plan.py holds this copy against the
    header) for `hashes` -> dict: B, composite, n (occurrences per bucket), bucket (of every hash), fill (per bucket: the fullest sub-range of the body that runs it — 128 sub-ranges up to 128 occurrences,
    256 above)."""
    n_all = len(hashes)
    thr = (2**64 - 1) // c
    sh = max(0, thr.bit_length() - 32)
    B = min(max(1, n_all // target), 1 << 24)
    hs_max = thr >> sh
    mult = min(0xFFFFFFFF, (B << 32) // (hs_max + 1))
    range_hs = (2**32 + mult - 1) // max(1, mult) + 1
    composite = mult >= 1 and range_hs.bit_length() + sh <= 64 - IDX_BITS
    hs = hashes >> np.uint64(sh)                                                    # < 2^32, like mult: the products fit 64 bits
    bucket = np.minimum((hs * np.uint64(mult)) >> np.uint64(32), np.uint64(B - 1)).astype(np.int64)
    n = np.bincount(bucket, minlength=B)
    fill = np.zeros(B, dtype=np.int64)
    if composite:
        lo = np.array([((b << 32) + mult - 1) // mult for b in range(B)], dtype=np.uint64)      # lowest hs of every bucket
        res = hs - lo[bucket]
        for cap in (LANE_CAP, 256):
            of_cap = (n[bucket] <= LANE_CAP) == (cap == LANE_CAP)
            sub_mult = ((cap << 32) // range_hs) if range_hs > cap else 0
            sub = np.minimum((res * np.uint64(sub_mult)) >> np.uint64(32) if sub_mult else res, np.uint64(cap - 1)).astype(np.int64)
            per = np.bincount((bucket * 256 + sub)[of_cap], minlength=B * 256).reshape(B, 256).max(axis=1)
            fill = np.maximum(fill, per)
    return dict(B=B, composite=composite, n=n, bucket=bucket, fill=fill)


# ---- a10: the filter dedup's hashes restated in numpy (sylph_amd/csrc/a10_plan.h; tests/test_oracle.py holds them against the model's
# walk, tests/test_a10_plan.py the header against them) ----
_FX_K = np.uint64(0x517cc1b727220a95)
_GOLD = np.uint64(0x9E3779B97F4A7C15)


def _fx_add(h, w):
    with np.errstate(over="ignore"):
        return (((h << np.uint64(5)) | (h >> np.uint64(59))) ^ w) * _FX_K


def a10_item_hash(km, marker):
    z = np.zeros_like(km)
    with np.errstate(over="ignore"):
        return _fx_add(_fx_add(_fx_add(z, km), marker & np.uint64(0xffffffff)), marker >> np.uint64(32)) * _GOLD


def a10_filter_geometry(fpr_j, cap_j):
    """-> (fingerprint bits, buckets) of a filter of that capacity and false-positive probability"""
    fp_bits = min(31, max(1, int(np.ceil(np.log2(1.0 / fpr_j) + np.log2(8.0)))))
    nb = 1
    while nb * 4 < cap_j:
        nb <<= 1
    return fp_bits, nb


def a10_reduced_key(h, fpr_j, cap_j):
    """(fingerprint, smaller of the item's two buckets): what a cuckoo filter can still tell apart (a10.hip header)"""
    fp_bits, nb = a10_filter_geometry(fpr_j, cap_j)
    f = (h >> np.uint64(32)) & np.uint64((1 << fp_bits) - 1)
    f = np.where(f == 0, np.uint64(1), f)
    i1 = h & np.uint64(nb - 1)
    i2 = (i1 ^ (_fx_add(np.zeros_like(f), f) >> np.uint64(11))) & np.uint64(nb - 1)
    return (f << np.uint64(32)) | np.minimum(i1, i2)


def build_path(stem, deps, suffix=""):
    """Where a test keeps what it compiles from `deps` (sources first, then the headers they include): a file in the temporary
    directory named after the CONTENTS of deps, so that a binary left there by another commit's sources is never taken for this one's.
    -> (path, whether it has to be built)"""
    import hashlib
    import tempfile
    h = hashlib.sha256()
    for p in deps:
        with open(p, "rb") as f:
            h.update(f.read())
    out = os.path.join(tempfile.gettempdir(), f"{stem}_{os.getuid()}_{h.hexdigest()[:16]}{suffix}")
    return out, not os.path.exists(out)
