#!/usr/bin/env python3
"""Static census of the k-mer loops: for every kernel of the given gfx950 assembly files (hipcc -O3 --offload-arch=gfx950
--offload-device-only -S), the innermost loop with the most vector instructions — the hash loop of reads_kernel and of the position
kernel — with its VALU count, its v_mov count and the instructions the hash spelling decides.  No GPU needed.
Usage: python tools/hash_loop_census.py reads.s seeds.s [--filter reads_kernel]"""
import collections, re, subprocess, sys

args = [a for a in sys.argv[1:] if not a.startswith("--")]
flt = sys.argv[sys.argv.index("--filter") + 1] if "--filter" in sys.argv else ""
args = [a for a in args if a != flt]
WATCH = ("v_mov_b32", "v_mad_u64_u32", "v_mul_lo_u32", "v_lshl_add_u64", "v_lshlrev_b64", "v_lshrrev_b64", "v_bitop3_b32", "v_cmp_lt_u64", "v_cmp_lt_u32", "v_min_f64", "v_bfe_u32", "v_cndmask_b32", "s_nop")


def demangle(n):
    d = subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip()
    d = re.sub(r"\(anonymous namespace\)::|sylph::", "", d)
    return re.sub(r"\(.*", "", d).replace("void ", "")


print(f'{"kernel":34s} {"loop":>12s} {"insts":>5s} {"VALU":>5s} ' + " ".join(f"{w[2:]:>12s}" for w in WATCH))
for path in args:
    lines = open(path).read().splitlines()
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if not m or f".type\t{m.group(1)},@function" not in "\n".join(lines[max(0, i - 6):i]):
            i += 1
            continue
        name, body, i = m.group(1), [], i + 1
        while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
            body.append(lines[i].split(";")[0].rstrip())
            i += 1
        label_at = {mm.group(1): n for n, l in enumerate(body) if (mm := re.match(r"^(\.LBB\d+_\d+):", l))}
        loops = []
        for n, l in enumerate(body):
            mm = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
            if mm and label_at.get(mm.group(1), n) < n:
                loops.append((label_at[mm.group(1)], n, mm.group(1)))
        inner = [lp for lp in loops if not any(o is not lp and lp[0] <= o[0] and o[1] <= lp[1] for o in loops)]
        best = None
        for a, b, lab in inner:
            ops = [re.sub(r"_(e32|e64|dpp|sdwa)$", "", l.split()[0]) for l in body[a:b + 1] if l.startswith("\t") and not l.strip().startswith(".")]
            valu = sum(o.startswith("v_") for o in ops)
            if best is None or valu > best[1]:
                best = (lab, valu, ops)
        kn = demangle(name)
        if best and flt in kn:
            h = collections.Counter(best[2])
            print(f"{kn[:34]:34s} {best[0]:>12s} {len(best[2]):5d} {best[1]:5d} " + " ".join(f"{h[w]:12d}" for w in WATCH))
