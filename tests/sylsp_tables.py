"""Entry streams of .sylsp tables for the tests of the device unpack (tests/test_sylsp_plan.py on the CPU, tests/test_gpu_sylsp.py
and tests/test_gpu_cli_sylsp.py on the GPU), and the numpy model every road is held against: a stable argsort by key, the last
entry of each run of equal keys kept — what rebuilding the reference's map by insertion gives (types.rs:117-129)."""
import numpy as np

T = 256                                           # sylsp_plan.h TILE (tests/test_sylsp_plan.py checks the constant)
SIZES = [0, 1, 2, T - 1, T, T + 1, 2 * T + 1]
MANY = 70_001                                     # many workgroups, more than one block of the radix sort
CASE_KINDS = ["ascending", "permutation", "duplicates"]
ENTRY = np.dtype([("kmer", "<u8"), ("count", "<u4")])
assert ENTRY.itemsize == 12


def pack_entries(kmers, counts):
    """-> uint8 array of len(kmers) * 12 bytes: the entries as bincode writes a Vec<(u64, u32)>"""
    e = np.zeros(len(kmers), dtype=ENTRY)
    e["kmer"], e["count"] = kmers, counts
    return e.view(np.uint8).reshape(-1)


def model_table(kmers, counts):
    kmers, counts = np.asarray(kmers, dtype=np.uint64), np.asarray(counts, dtype=np.uint32)
    order = np.argsort(kmers, kind="stable")
    sk, sc = kmers[order], counts[order]
    last = np.ones(len(sk), dtype=bool)
    last[:-1] = sk[1:] != sk[:-1]
    return sk[last], sc[last]


def entries_case(kind, n, seed=0):
    """n entries: `ascending` (strictly; what write_sylsp writes), `permutation` (the same keys in random order, standing in for
    hashbrown's), `duplicates` (a permutation with 1 % of the keys — at least one — repeated, one of the repeats ending on a count
    of 0).  From two entries on, the keys 0 and 2^64 - 1 and the counts 0 and 2^32 - 1 are among them."""
    rng = np.random.default_rng(1000 * n + seed)
    kmers = np.unique(rng.integers(1, 2**64 - 1, size=n + 64, dtype=np.uint64))[:n]
    assert len(kmers) == n
    counts = rng.integers(1, 1000, size=n).astype(np.uint32)
    if n >= 2:
        kmers[0], kmers[-1] = 0, 2**64 - 1
        counts[0], counts[-1] = 0, 2**32 - 1
    if kind == "ascending":
        return kmers, counts
    perm = rng.permutation(n)
    if n >= 2 and (perm == np.arange(n)).all():
        perm = perm[::-1].copy()
    kmers, counts = kmers[perm], counts[perm]
    if kind == "permutation" or n < 2:
        return kmers, counts
    assert kind == "duplicates"
    n_dup = max(1, n // 100)
    dst = rng.choice(n, size=n_dup, replace=False)
    src = (dst + rng.integers(1, n, size=n_dup)) % n                       # another entry's key
    kmers = kmers.copy()
    kmers[dst] = kmers[src]
    last_of_first = max(int(dst[0]), int(src[0]))                          # the later of the two in file order (unless a third repeats it)
    counts[last_of_first] = 0
    return kmers, counts
