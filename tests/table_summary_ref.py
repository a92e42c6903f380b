"""What the table-summary tests share: an independent restatement of the walk (contain.rs:901-951 as the host walks it, in integers),
the summary's layout, and the seeded tables of the issue's simulation."""
import ctypes as C

import numpy as np

FIELDS = ("median_sum", "total_counts", "steps", "num_1s", "num_not1s", "max_state", "flags", "rung", "open_chunks", "reserved")
DECLINED, DECLINED_LADDER, DECLINED_SUM, DECLINED_SIZE = 1, 2, 4, 8
WALK_FIELDS = ("median_sum", "total_counts", "steps", "num_1s", "num_not1s", "max_state")


class Summary(C.Structure):
    _fields_ = [("median_sum", C.c_uint64), ("total_counts", C.c_uint64)] + [(f, C.c_uint32) for f in FIELDS[2:]]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f in FIELDS}


def walk(counts):
    """the plain walk -> the six integers"""
    m = median_sum = steps = max_state = 0
    for x in np.asarray(counts).tolist():
        if x > 1:
            m += 1 if x > m else -1
            median_sum += m
            steps += 1
            max_state = max(max_state, m)
    c = np.asarray(counts, dtype=np.uint64)
    return dict(median_sum=median_sum, total_counts=int(c.sum(dtype=np.uint64)), steps=steps, num_1s=int((c == 1).sum()),
                num_not1s=int(c[c != 1].sum(dtype=np.uint64)) & 0xFFFFFFFF, max_state=max_state)


def mov_avg_median(s):
    return float(s["median_sum"]) / (1.0 + s["steps"])


def family(seed, depth, n=400_000, sigma=0.5, ones=0.0):
    """n counts: Poisson of a log-normal depth around `depth`, zeros lifted to 1, a share `ones` forced to 1 (error k-mers), 1 in 5,000
    entries an outlier of 5*10^4 .. 2*10^6"""
    rng = np.random.default_rng(seed)
    lam = depth * rng.lognormal(0.0, sigma, size=n)
    c = np.maximum(rng.poisson(lam), 1).astype(np.uint32)
    if ones:
        c[rng.random(n) < ones] = 1
    out = rng.random(n) < 1 / 5000
    c[out] = rng.integers(50_000, 2_000_001, size=int(out.sum()), dtype=np.uint32)
    return c


# (name, seed, depth, share of ones): the state hovers near 3, 9 and 400
FAMILIES = (("near3", 11, 3.0, 0.3), ("near9", 12, 9.5, 0.2), ("near400", 13, 430.0, 0.5))
