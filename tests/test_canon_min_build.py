"""The read kernel picks the canonical k-mer with one v_min_f64 (min_u62, csrc/device_common.h): two values below 2^62 are non-negative
finite doubles, whose order is the unsigned order of their bits — as long as the hardware does not flush denormals (a k-mer with five or
more leading A is one; every 21-mer is).  No GPU needed: the build's flags must leave FLOAT_DENORM_MODE_16_64 = 3 in the kernel
descriptors (a probe kernel's and every one of csrc/reads.hip), and the windows kmer_step builds right-aligned (fword / rword /
v_bfe_u32) are held against the left-aligned ones of the earlier spelling and against the k-mers read off the bases, in a Python model, for every T and both K."""
import os
import re
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sylph_amd", "csrc")
M32 = 0xFFFFFFFF

PROBE = r"""
#include "device_common.h"
using namespace sylph;
__global__ void probe_min_u62(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, uint64_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = min_u62(a[i], b[i]);
}
"""


def makefile_var(name):
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    return re.search(rf"^{name} \?= (.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()


def test_min_u62_compiles_with_f64_denormals_preserved(tmp_path):
    src, asm = tmp_path / "probe.hip", tmp_path / "probe.s"
    src.write_text(PROBE)
    hipcc = os.environ.get("HIPCC") or makefile_var("HIPCC")[0]
    subprocess.check_call([hipcc, *makefile_var("CXXFLAGS"), "-I", CSRC, "--offload-device-only", "-S", str(src), "-o", str(asm)])
    text = asm.read_text()
    assert re.search(r"^\s*v_min_f64(_e\d+)?\s", text, re.M)
    modes = re.findall(r"\.amdhsa_float_denorm_mode_16_64\s+(\d+)", text)
    assert modes == ["3"], modes                     # one kernel, denormals neither flushed on input nor on output


def test_every_kernel_of_reads_hip_keeps_f64_denormals(tmp_path):
    """The kernels that run min_u62 themselves: no descriptor of csrc/reads.hip may say anything but 3 (a per-kernel attribute or a
    flag of that file alone would not show in the probe above)."""
    asm = tmp_path / "reads.s"
    hipcc = os.environ.get("HIPCC") or makefile_var("HIPCC")[0]
    subprocess.check_call([hipcc, *makefile_var("CXXFLAGS"), "--offload-device-only", "-S", os.path.join(CSRC, "reads.hip"), "-o", str(asm)])
    text = asm.read_text()
    modes = re.findall(r"\.amdhsa_float_denorm_mode_16_64\s+(\d+)", text)
    assert len(modes) >= 20 and set(modes) == {"3"}, modes
    assert len(re.findall(r"^\s*v_min_f64(_e\d+)?\s", text, re.M)) >= 16 * 20       # 16 per hot loop of every reads_kernel instance


def test_double_order_is_unsigned_order_below_2_62():
    rng = np.random.default_rng(62)
    edge = [0, 1, 2, (1 << 52) - 1, 1 << 52, (1 << 52) + 1, (1 << 62) - 1, (1 << 62) - 2, 1 << 32, (1 << 32) - 1, (1 << 42) - 1, (1 << 20) - 1]
    vals = edge + [int(x) >> int(s) for x, s in zip(rng.integers(0, 1 << 62, size=4000), rng.integers(0, 62, size=4000))]
    as_double = [struct.unpack("<d", struct.pack("<Q", v))[0] for v in vals]
    assert all(d == d and d >= 0.0 and d != float("inf") for d in as_double)
    order = sorted(range(len(vals)), key=lambda i: vals[i])
    for i, j in zip(order, order[1:]):
        assert (as_double[i] < as_double[j]) == (vals[i] < vals[j]) and (as_double[i] == as_double[j]) == (vals[i] == vals[j])


# ------------------------------------------------------------------------------------------------ the windows, modelled
def alignbit(hi, lo, s):
    return (((hi << 32) | lo) >> (s & 31)) & M32


def ubfe(x, off, width):
    return (x >> off) & ((1 << width) - 1)


def rcword(a):
    r = int(f"{a:032b}"[::-1], 2)
    return ~(((r & 0x55555555) << 1) | ((r >> 1) & 0x55555555)) & M32


def fword(P, A0, A1, A2):
    return A0 if P == 0 else alignbit(A0, A1, 32 - P) if P < 32 else A1 if P == 32 else alignbit(A1, A2, 64 - P) if P < 64 else A2


def rword(Q, B0, B1, B2):
    return B0 if Q == 0 else alignbit(B1, B0, Q) if Q < 32 else B1 if Q == 32 else alignbit(B2, B1, Q - 32) if Q < 64 else B2


def clean_windows(K, T, A, B):
    """kmer_step today: (forward, reverse complement), right-aligned, tops zero."""
    HB, T0 = 2 * K - 32, T & ~1
    if 2 * T + HB <= 32:                                   # the field lies inside A0 / B1
        fhi, rhi = ubfe(A[0], 32 - HB - 2 * T, HB), ubfe(B[1], 2 * T, HB)
    else:
        cf, cr = fword(2 * T0, *A), rword(2 * T0 + 32, *B)
        fhi, rhi = ubfe(cf, 32 - HB - 2 * (T - T0), HB), ubfe(cr, 2 * (T - T0), HB)
    return (fhi << 32) | fword(2 * T + HB, *A), (rhi << 32) | rword(2 * T, *B)


def left_aligned_windows(K, T, A, Bm, B):
    """kmer_step up to round 12: both k-mers in the top 2K bits, garbage below."""
    D = 64 - 2 * K
    A0, A1, A2 = A
    B0, B1, B2 = B
    fhi, flo = (A0, A1) if T == 0 else (alignbit(A0, A1, 32 - 2 * T), alignbit(A1, A2, 32 - 2 * T))
    OFF = 2 * T - D
    if OFF < 0:
        rlo, rhi = alignbit(B0, Bm, OFF + 32), alignbit(B1, B0, OFF + 32)
    elif OFF == 0:
        rlo, rhi = B0, B1
    else:
        rlo, rhi = alignbit(B1, B0, OFF), alignbit(B2, B1, OFF)
    return (fhi << 32) | flo, (rhi << 32) | rlo


def test_clean_windows_equal_the_left_aligned_ones_and_the_bases():
    rng = np.random.default_rng(13)
    special = [(0, 0, 0), (M32, M32, M32), (0, M32, 0), (M32, 0, M32), (0x55555555, 0xAAAAAAAA, 0x33333333)]
    cases = special + [tuple(int(x) for x in rng.integers(0, 1 << 32, size=3)) for _ in range(400)]
    for A in cases:
        Bm, B = rcword(int(rng.integers(0, 1 << 32))), tuple(rcword(a) for a in A)
        codes = [(w >> (30 - 2 * j)) & 3 for w in A for j in range(16)]
        for K in (21, 31):
            D = 64 - 2 * K
            for T in range(16):
                f, r = clean_windows(K, T, A, B)
                fl, rl = left_aligned_windows(K, T, A, Bm, B)
                assert (f, r) == (fl >> D, rl >> D), (K, T, A)
                assert f < (1 << 62) and r < (1 << 62)
                assert min(f, r) == (fl if fl < rl else rl) >> D
                fwd = rev = 0
                for j in range(K):
                    fwd = (fwd << 2) | codes[T + j]
                    rev = (rev << 2) | (3 - codes[T + K - 1 - j])
                assert (f, r) == (fwd, rev), (K, T, A)
