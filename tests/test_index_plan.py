"""CPU tests of the line index's arithmetic (sylph_amd/csrc/index_plan.h, the very header line_index.hip, contain_index.h and hits.hip
include, compiled with g++ through tests/index_plan_capi.cpp, once per line size): the bucket division against divmod, the geometry
and its refusals, the pass split, the slot codec, a model index built with the plan's bucket writer and looked up with the plan's slot
scan against a dictionary, the hit key rules — and the model's stand-alone sanitizer run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from .helpers import build_path

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "sylph_amd", "csrc")
HDR = os.path.join(CSRC, "index_plan.h")
M64 = 2**64 - 1
BUILDABLE, TOO_MANY_GENOMES, TOO_MANY_BUCKETS = 0, 1, 2
u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p


def load(slots):
    src = os.path.join(HERE, "index_plan_capi.cpp")
    out, stale = build_path(f"sylph_index_plan{slots}", [src, HDR], ".so")
    if stale:
        tmp = out + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-DSYLPH_LINE_SLOTS={slots}", "-shared", "-fPIC", "-o", tmp, src])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    lib.ip_constants.argtypes = [vp]
    lib.ip_magic.restype = u64
    lib.ip_magic.argtypes = [u64]
    lib.ip_bucket_rem.argtypes = [vp, vp, u64, vp, vp]
    lib.ip_geometry.argtypes = [u64, u64, u64, u64, u64, vp]
    lib.ip_overflow_fits.argtypes = [u64, C.c_int]
    lib.ip_n_passes.restype = u32
    lib.ip_n_passes.argtypes = [u64, u64, u64]
    lib.ip_pass_of.argtypes = [u32, u32, u64, u64, u64, u64, vp]
    lib.ip_encode_posting.restype = u64
    lib.ip_encode_posting.argtypes = [u64, u32, C.c_int]
    lib.ip_encode_descriptor.restype = u64
    lib.ip_encode_descriptor.argtypes = [u64, u64, C.c_int]
    lib.ip_decode.argtypes = [u64, C.c_int, vp]
    lib.ip_layout.argtypes = [u32, vp]
    lib.ip_hit_key.restype = u64
    lib.ip_hit_key.argtypes = [u64, u32]
    lib.ip_compact_key.argtypes = [u32, u64, vp]
    lib.ip_coverage_width.restype = u32
    lib.ip_coverage_width.argtypes = [C.c_int, u32]
    lib.ip_model_build.restype = vp
    lib.ip_model_build.argtypes = [vp, vp, u64, u64, u64, u64, u64, u64]
    lib.ip_model_free.argtypes = [vp]
    lib.ip_model_info.argtypes = [vp, vp]
    lib.ip_model_lines.restype = C.POINTER(u64)
    lib.ip_model_lines.argtypes = [vp]
    lib.ip_model_ovf.restype = C.POINTER(u64)
    lib.ip_model_ovf.argtypes = [vp]
    lib.ip_model_lookup.restype = u64
    lib.ip_model_lookup.argtypes = [vp, u64, vp, u64, vp]
    k = np.zeros(4, dtype=np.uint64)
    lib.ip_constants(k.ctypes.data)
    lib.SLOTS, lib.LONG_RUN_MIN, lib.LAMBDA = int(k[0]), int(k[1]), int(k[2])
    assert lib.SLOTS == slots and int(k[3]) == M64
    return lib


@pytest.fixture(scope="module")
def L():
    return load(8)


@pytest.fixture(scope="module", params=[8, 4])
def LS(request):
    return load(request.param)


def geometry(L, n_genomes, kmer_lo, max_key, postings, lam):
    o = np.zeros(7, dtype=np.uint64)
    L.ip_geometry(n_genomes, kmer_lo, max_key, postings, lam, o.ctypes.data)
    return dict(zip(("why", "gb", "gshift", "div_cap", "div", "magic", "n_buckets"), (int(v) for v in o)))


def bucket_rem(L, xs, divs):
    x, d = np.array(xs, dtype=np.uint64), np.array(divs, dtype=np.uint64)
    q, r = np.zeros(len(x), dtype=np.uint64), np.zeros(len(x), dtype=np.uint64)
    L.ip_bucket_rem(x.ctypes.data, d.ctypes.data, len(x), q.ctypes.data, r.ctypes.data)
    return q, r


def rand64(rng, n=None):
    return rng.integers(0, 2**64, size=n, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------------------------- division
def test_bucket_rem_equals_divmod(L):
    rng = np.random.default_rng(11)
    xs, ds = [], []
    for gb in (1, 5, 20, 30):
        div_cap = 2**(63 - gb) - 1
        divs = [2, 3, 2**32 - 1, 2**32, 2**32 + 1, div_cap - 1, div_cap] + [int(v) % (div_cap - 1) + 2 for v in rand64(rng, 20)]
        for div in divs:
            assert 2 <= div <= div_cap
            last = M64 // div * div
            for x in [0, 1, div - 1, div, div + 1, M64 - 1, M64, last, last - 1] + [int(v) for v in rand64(rng, 20)]:
                xs.append(x)
                ds.append(div)
    # 10^5 random pairs, the divisor's magnitude spread over 2 .. 2^62 bits
    bits = rng.integers(2, 63, size=10**5)
    rd = [int(v) % (2**int(b) - 2) + 2 for v, b in zip(rand64(rng, 10**5), bits)]
    xs += [int(v) for v in rand64(rng, 10**5)]
    ds += rd
    q, r = bucket_rem(L, xs, ds)
    for x, d, qq, rr in zip(xs, ds, q.tolist(), r.tolist()):
        assert (qq, rr) == divmod(x, d), (x, d)
    q, r = bucket_rem(L, [0, 5, M64], [1, 1, 1])                       # div == 1: the bucket is the value
    assert q.tolist() == [0, 5, M64] and r.tolist() == [0, 0, 0] and L.ip_magic(1) == 0 and L.ip_magic(2) == 2**63


# ------------------------------------------------------------------------------------------------------------------- geometry
def check_geometry(L, n_genomes, kmer_lo, max_key, postings, lam, rng):
    g = geometry(L, n_genomes, kmer_lo, max_key, postings, lam)
    assert g["why"] == BUILDABLE, g
    gb = max(1, (max(n_genomes, 1) - 1).bit_length())
    assert g["gb"] == gb and g["gshift"] == gb + 1 and g["div_cap"] == 2**(63 - gb) - 1
    assert 1 <= g["div"] <= g["div_cap"] and g["magic"] == L.ip_magic(g["div"]) == (2**64 // g["div"] if g["div"] > 1 else 0)
    assert g["n_buckets"] == (max_key - kmer_lo) // g["div"] + 1 < 2**32 - 1
    keys = [kmer_lo, max_key] + [kmer_lo + int(v) % (max_key - kmer_lo + 1) for v in rand64(rng, 50)]
    q, r = bucket_rem(L, [k - kmer_lo for k in keys], [g["div"]] * len(keys))
    assert (q < g["n_buckets"]).all() and (r < g["div"]).all()
    # neither the largest posting slot nor the largest descriptor is the empty pattern
    assert L.ip_encode_posting(g["div"] - 1, 2**gb - 1, g["gshift"]) != M64
    assert L.ip_encode_descriptor(2**(62 - gb) - 1, M64, g["gshift"]) != M64
    assert L.ip_overflow_fits(2**(62 - gb) - 1, gb) and not L.ip_overflow_fits(2**(62 - gb), gb)
    return g


def test_geometry(L):
    rng = np.random.default_rng(12)
    for _ in range(300):
        n_genomes = int(rng.choice([0, 1, 2, 3, 32, 33, 2**20, 2**30, int(rng.integers(1, 2**30))]))
        lo = int(rand64(rng)) >> int(rng.integers(0, 64))
        hi = lo + (int(rand64(rng)) >> int(rng.integers(0, 64))) % (M64 - lo + 1)
        postings = int(rng.integers(1, 2**33))
        lam = int(rng.choice([0, 1, 2, 3, 4, 8]))
        g = geometry(L, n_genomes, lo, hi, postings, lam)
        if g["why"] == TOO_MANY_BUCKETS:                               # (a wide range with billions of postings)
            assert g["n_buckets"] >= 2**32 - 1
            continue
        check_geometry(L, n_genomes, lo, hi, postings, lam, rng)
    for gb_genomes in (2, 32, 2**20, 2**30):                            # the wrapped span: max_key - kmer_lo + 1 == 2^64
        g = check_geometry(L, gb_genomes, 0, M64, 1000, 4, rng)
        assert g["div"] == g["div_cap"]
    g = check_geometry(L, 10, 100, 100 + 999, 1000, 1, rng)            # a dense range, one posting per bucket aimed for
    assert g["div"] == 1 and g["magic"] == 0 and g["n_buckets"] == 1000
    g = check_geometry(L, 10, 7, 7, 1, 0, rng)                         # one k-mer
    assert g["div"] == 1 and g["n_buckets"] == 1
    assert check_geometry(L, 10, 0, 4000, 1000, 0, rng)["div"] == -(-4001 // (1000 // L.LAMBDA))   # lambda 0: the line size's default
    # the three refusals
    assert geometry(L, 2**30, 0, 10**6, 1000, 4)["why"] == BUILDABLE and geometry(L, 2**30 + 1, 0, 10**6, 1000, 4)["why"] == TOO_MANY_GENOMES
    assert geometry(L, M64, 0, 10**6, 1000, 4)["why"] == TOO_MANY_GENOMES
    g = geometry(L, 100, 0, 2**63, 2**34, 1)
    assert g["why"] == TOO_MANY_BUCKETS and g["n_buckets"] == 2**63 // g["div"] + 1 >= 2**32 - 1
    assert L.ip_overflow_fits(2**57 - 1, 5) and not L.ip_overflow_fits(2**57, 5)


# ------------------------------------------------------------------------------------------------------------------- pass split
def check_passes(L, n_buckets, n_pass, kmer_lo, kmer_hi, div):
    o = np.zeros(4, dtype=np.uint64)
    at = 0
    for p in range(n_pass):
        L.ip_pass_of(p, n_pass, n_buckets, kmer_lo, kmer_hi, div, o.ctypes.data)
        b0, b1, klo, khi = (int(v) for v in o)
        assert b0 == at and b1 > b0                                    # no gap, no overlap, no empty pass (n_pass <= n_buckets)
        assert klo == kmer_lo + b0 * div <= M64                        # (Python integers: the sum itself stays below 2^64)
        if p + 1 < n_pass:
            assert khi == kmer_lo + b1 * div <= M64 and khi > klo
        else:
            assert khi == kmer_hi                                      # the shard's own bound; 0 = open
        at = b1
    assert at == n_buckets


def test_pass_split(L):
    rng = np.random.default_rng(13)
    for n_buckets, passes in [(1, 1), (5, 5), (7, 3), (1000, 7)] + [(int(rng.integers(1, 10**6)), int(rng.integers(1, 50))) for _ in range(100)]:
        passes = min(passes, n_buckets)
        assert L.ip_n_passes(n_buckets, passes * 10, 10) == passes and L.ip_n_passes(n_buckets, passes * 10 - 9, 10) == passes
        for kmer_hi in (0, 10**15):
            check_passes(L, n_buckets, passes, 12345, kmer_hi, int(rng.integers(1, 10**9)))
    assert L.ip_n_passes(5, 1000, 10) == 5 and L.ip_n_passes(5, 0, 10) == 1 and L.ip_n_passes(100, 50, 0) == 50   # capped by the buckets; at least one; pass_max 0 reads as 1
    for genomes in (2, 32, 2**30):                                      # up to the last value: max_key = 2^64 - 1
        g = geometry(L, genomes, 0, M64, 1000, 4)
        for passes in (1, 3, 7):
            check_passes(L, g["n_buckets"], min(passes, g["n_buckets"]), 0, 0, g["div"])
        g = geometry(L, genomes, 2**63 + 5, M64, 10**6, 4)
        check_passes(L, g["n_buckets"], min(7, g["n_buckets"]), 2**63 + 5, 0, g["div"])


# ------------------------------------------------------------------------------------------------------------------- slot codec
def test_slot_codec_and_bucket_layout(LS):
    o = np.zeros(5, dtype=np.uint64)
    for gb in (1, 5, 20, 30):
        gshift, gmask = gb + 1, 2**gb - 1
        for rem, genome in ((0, 0), (1, gmask), (2**(63 - gb) - 2, gmask), (12345, 1)):
            s = LS.ip_encode_posting(rem, genome, gshift)
            LS.ip_decode(s, gshift, o.ctypes.data)
            assert (int(o[0]), int(o[1]), int(o[2])) == (rem, 0, genome)
        for start, length in ((0, 1), (5, gmask - 1), (5, gmask), (2**(62 - gb) - 1, gmask + 1), (77, 10**9)):
            s = LS.ip_encode_descriptor(start, length, gshift)
            LS.ip_decode(s, gshift, o.ctypes.data)
            assert (int(o[1]), int(o[3]), int(o[4])) == (1, start, min(length, gmask))        # the run length saturates
    o2 = np.zeros(2, dtype=np.uint32)
    S = LS.SLOTS
    for c, want in ((0, (0, 0)), (1, (1, 0)), (S - 1, (S - 1, 0)), (S, (S, 0)), (S + 1, (S - 1, 3)), (S + 200, (S - 1, 202))):
        LS.ip_layout(c, o2.ctypes.data)
        assert tuple(o2.tolist()) == want, c                           # (what overflows, and the closing sentinel)


# ------------------------------------------------------------------------------------------------------------------- model index
class Model:
    def __init__(self, L, keys, gids, n_genomes, lam, pass_max, kmer_lo=0, kmer_hi=0):
        order = np.lexsort((gids, keys))                              # the build's stable sort of genome-major postings
        self.L, self.keys, self.gids = L, np.ascontiguousarray(keys[order]), np.ascontiguousarray(gids[order].astype(np.uint32))
        self.h = L.ip_model_build(self.keys.ctypes.data, self.gids.ctypes.data, len(keys), n_genomes, kmer_lo, kmer_hi, lam, pass_max)
        assert self.h
        o = np.zeros(5, dtype=np.uint64)
        L.ip_model_info(self.h, o.ctypes.data)
        self.n_buckets, self.n_ovf, self.n_pass, self.div, self.gshift = (int(v) for v in o)
        self.base = kmer_lo
        self.want = {}
        for k, g in zip(self.keys.tolist(), self.gids.tolist()):
            self.want.setdefault(k, []).append(g)
        self.bucket_rems = {}
        for k in self.keys.tolist():
            self.bucket_rems.setdefault((k - kmer_lo) // self.div, []).append((k - kmer_lo) % self.div)
        self.buf = np.zeros(len(keys) + 1, dtype=np.uint32)

    def lookup(self, km):
        flag = C.c_int(0)
        n = self.L.ip_model_lookup(self.h, km, self.buf.ctypes.data, len(self.buf), C.byref(flag))
        return self.buf[:n].tolist(), flag.value

    def long_expected(self, km):
        """the scan hands the run back exactly when the rest of the bucket is relevant and its STORED length reaches LONG_RUN_MIN"""
        if km < self.base:
            return 0
        S, rems = self.L.SLOTS, self.bucket_rems.get((km - self.base) // self.div, [])
        if len(rems) <= S or rems[S - 2] > (km - self.base) % self.div:
            return 0
        return int(min(len(rems) - (S - 1), 2**(self.gshift - 1) - 1) >= self.L.LONG_RUN_MIN)

    def check(self, queries):
        n_long = 0
        for km in queries:
            got, long_run = self.lookup(km)
            assert got == self.want.get(km, []), km                    # the dictionary's genomes, ascending, repeats kept
            assert long_run == self.long_expected(km), km
            n_long += long_run
        lines = np.ctypeslib.as_array(self.L.ip_model_lines(self.h), shape=(self.n_buckets, self.L.SLOTS))
        in_line = sum(min(len(r), self.L.SLOTS if len(r) <= self.L.SLOTS else self.L.SLOTS - 1) for r in self.bucket_rems.values())
        crowded = sum(1 for r in self.bucket_rems.values() if len(r) > self.L.SLOTS)
        assert int((lines != M64).sum()) == in_line + crowded          # every other slot is the empty pattern
        assert self.n_ovf == len(self.keys) - in_line + crowded        # the overflowing postings and one sentinel per run
        return n_long

    def close(self):
        self.L.ip_model_free(self.h)


def crowded_case(L, gb, rng):
    """Postings over the whole 2^64 range (the keys 0 and 2^64 - 1 are in: the span wraps, div is div_cap) with buckets of exactly
    0, 1, 7, 8, 9, 7 + 47, 7 + 48, 7 + 64, 7 + 65 and 7 + 200 postings, and the same around this build's line size; three k-mers
    (remainders) per crowded bucket, genome ids drawn with repeats.  -> keys, gids, n_genomes, queries"""
    n_genomes = 2**gb
    div = 2**(63 - gb) - 1
    S = L.SLOTS
    sizes = sorted(set([0, 1, 7, 8, 9, 7 + 47, 7 + 48, 7 + 64, 7 + 65, 7 + 200] + [S - 1, S, S + 1] + [S - 1 + r for r in (47, 48, 64, 65, 200)]))
    keys, gids, queries = [0, M64], [3, 3], [0, M64, 1, M64 - 1]
    for i, c in enumerate(sizes):
        b = 2 + 2 * i                                                  # every other bucket stays empty
        t_b, t_c = c // 3, c // 5
        for rem, t in ((5, c - t_b - t_c), (6, t_b), (1000, t_c)):
            keys += [b * div + rem] * t
            gids += sorted(int(g) for g in rng.integers(0, n_genomes, size=t))
        queries += [b * div + rem for rem in (0, 4, 5, 6, 7, 500, 1000, 1001, div - 1)] + [(b + 1) * div + 5]
    assert (2 + 2 * len(sizes)) * div < M64 - div
    return np.array(keys, dtype=np.uint64), np.array(gids, dtype=np.uint32), n_genomes, queries


@pytest.mark.parametrize("gb", [5, 7, 8])
def test_model_index_of_crowded_buckets_equals_a_dictionary(LS, gb):
    """gb = 5: the descriptor's length field holds at most 31, every run is stored shorter than LONG_RUN_MIN and walked by the scan;
    gb = 7: 7 + 200 saturates at 127, still long; gb = 8: nothing saturates."""
    rng = np.random.default_rng(14)
    keys, gids, n_genomes, queries = crowded_case(LS, gb, rng)
    for pass_max in (1 << 30, 100):
        m = Model(LS, keys, gids, n_genomes, 4, pass_max)
        assert m.div == 2**(63 - gb) - 1 and m.gshift == gb + 1 and (m.n_pass > 1) == (pass_max == 100)
        n_long = m.check(queries)
        assert (n_long == 0) == (gb == 5)
        m.close()


def test_model_index_of_random_postings_equals_a_dictionary(LS):
    rng = np.random.default_rng(15)
    for trial in range(12):
        n_genomes = int(rng.choice([1, 2, 31, 300]))
        lo = int(rng.choice([0, 10**6, 2**63]))
        span = int(rng.choice([500, 10**5, 2**40]))
        pool = lo + rng.integers(0, span, size=400, dtype=np.uint64)
        keys = np.concatenate([rng.choice(pool, size=3000), pool[:3].repeat(150)])          # shared k-mers: crowded buckets
        gids = rng.integers(0, n_genomes, size=len(keys)).astype(np.uint32)
        lam, pass_max = int(rng.choice([0, 1, 2, 3, 8])), int(rng.choice([1 << 30, 777, 50]))
        m = Model(LS, keys, gids, n_genomes, lam, pass_max, kmer_lo=lo)
        absent = [lo + int(v) % (span * 2) for v in rand64(rng, 300)] + [0, lo - 1 if lo else 0, M64]
        m.check(sorted(set(keys.tolist())) + absent)
        m.close()
    keys = np.arange(100, 1100, dtype=np.uint64)                       # dense, lambda 1: div == 1, every remainder 0
    m = Model(LS, keys, (keys % 7).astype(np.uint32), 7, 1, 1 << 30, kmer_lo=100)
    assert m.div == 1 and m.n_buckets == 1000
    m.check(list(range(90, 1110)))
    m.close()


# ------------------------------------------------------------------------------------------------------------------- hit keys
def test_hit_key_rules(L):
    assert L.ip_hit_key(0, 0) == 0 and L.ip_hit_key(5, 7) == (5 << 32) | 7 and L.ip_hit_key(2**32 - 2, 2**32 - 1) == ((2**32 - 2) << 32) | (2**32 - 1)
    o = (C.c_int * 3)()
    for mc in (0, 1, 255, 256, 65535, 65536, 2**32 - 1):
        cb = max(1, mc.bit_length())
        assert L.ip_coverage_width(1, mc) == (1 if mc < 256 else 2 if mc < 65536 else 4) and L.ip_coverage_width(0, mc) == 4
        rows = [0, 1, 2**32 - 2]
        if cb < 32:
            rows += [2**(32 - cb) - 1, 2**(32 - cb), 2**(32 - cb) + 1, max(2**(31 - cb), 1)]   # both sides of cb + rb == 32
        for n_rows in rows:
            L.ip_compact_key(mc, n_rows, o)
            rb = max(1, n_rows.bit_length())
            assert (o[0], o[1], o[2]) == (cb, rb, int(cb + rb <= 32)), (mc, n_rows)
        if cb < 32:
            L.ip_compact_key(mc, 2**(32 - cb) - 1, o)
            assert o[2] == 1
            L.ip_compact_key(mc, 2**(32 - cb), o)
            assert o[2] == 0


# ------------------------------------------------------------------------------------------------------------------- sanitizers
@pytest.mark.parametrize("slots", [8, 4])
def test_standalone_program_runs_clean_under_the_sanitizers(tmp_path, slots):
    """tests/index_sanitize_main.cpp + the model, built with AddressSanitizer and UBSan into a program of its own and run on the CPU over
    the crowded-bucket case (gb = 5 and 8, one pass and several): nothing is loaded into this interpreter."""
    srcs = [os.path.join(HERE, f) for f in ("index_sanitize_main.cpp", "index_plan_capi.cpp")]
    exe, stale = build_path(f"sylph_index_sanitize{slots}", srcs + [HDR])
    if stale:
        tmp = exe + f".{os.getpid()}"
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                               "-Werror", f"-DSYLPH_LINE_SLOTS={slots}", "-o", tmp] + srcs)
        os.replace(tmp, exe)
    lib = load(slots)
    for gb in (5, 8):
        keys, gids, n_genomes, queries = crowded_case(lib, gb, np.random.default_rng(14))
        order = np.lexsort((gids, keys))
        for pass_max in (1 << 30, 100):
            path = tmp_path / f"case{gb}_{pass_max}.bin"
            with open(path, "wb") as f:
                f.write(np.array([len(keys), n_genomes, 4, pass_max, len(queries)], dtype=np.uint64).tobytes())
                f.write(keys[order].tobytes() + gids[order].astype(np.uint64).tobytes() + np.array(queries, dtype=np.uint64).tobytes())
            p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
            assert p.returncode == 0 and "index sanitize run ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
            assert ("0 long runs" in p.stdout) == (gb == 5)
