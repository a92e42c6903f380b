"""GPU tests of `sylph-hip profile` / `query` with the confidence intervals resampled on the device (SYLPH_HIP_BOOTSTRAP_DEVICE=only) against
the host's loop (=0): the same bytes on stdout.  Database and reads are tests/test_gpu_cli.py's (same slices, same simulation, same
seed); a thinned copy of the reads brings the genomes down to the coverage at which a lambda — and with it an interval — is estimated."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from .helpers import ACGT, random_seq, revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sylph_amd", "sylph-hip")


def run(*args, bootstrap=None):
    env = dict(os.environ)
    env["SYLPH_HIP_EXACT_DEDUP"] = "1"
    env.pop("SYLPH_HIP_BOOTSTRAP_DEVICE", None)
    if bootstrap is not None:
        env["SYLPH_HIP_BOOTSTRAP_DEVICE"] = bootstrap
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=env)


def write_fasta(path, records, gz=True, width=70):
    op = gzip.open if gz else open
    with op(path, "wb") as f:
        for name, seq in records:
            f.write(b">" + name + b"\n")
            s = bytes(seq)
            for i in range(0, len(s), width):
                f.write(s[i:i + width] + b"\n")


def write_fastq(path, reads, gz=False, prefix=b"r"):
    op = gzip.open if gz else open
    with op(path, "wb") as f:
        for i, s in enumerate(reads):
            f.write(b"@" + prefix + str(i).encode() + b" extra\n" + bytes(s) + b"\n+\n" + b"I" * len(s) + b"\n")


def build_inputs(d, golden_dir):
    """genomes, reads, thinned reads and the database (-c 50) under directory d (also what tools/bootstrap_bench.py times)"""
    z = np.load(os.path.join(golden_dir, "ecoli_slices.npz"))
    rng = np.random.default_rng(123)
    genomes = {}
    for gi, name in enumerate(("EC590", "K12", "O157")):
        b, off = z[f"g{gi}_bases"], z[f"g{gi}_off"]
        recs = [(f"{name}_contig{i} test genome".encode(), b[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]
        p = str(d / f"{name}.fasta.gz")
        write_fasta(p, recs)
        genomes[name] = (p, recs)
    unrelated = random_seq(rng, 120000)
    genomes["rand"] = (str(d / "rand.fa"), [(b"random_genome", unrelated)])
    write_fasta(genomes["rand"][0], genomes["rand"][1], gz=False)

    def sim(g, n):
        m1, m2 = [], []
        for _ in range(n):
            ins = int(rng.integers(200, 400))
            s = int(rng.integers(0, len(g) - ins))
            frag = g[s:s + ins] if rng.random() < 0.5 else revcomp(g[s:s + ins])
            a, b = frag[:100].copy(), revcomp(frag)[:100].copy()
            for m in (a, b):
                e = rng.random(100) < 0.01
                m[e] = rng.choice(ACGT, size=int(e.sum()))
            m1.append(a); m2.append(b)
        return m1, m2
    a1, a2 = sim(genomes["K12"][1][0][1], 9000)
    b1, b2 = sim(unrelated, 600)
    c1, c2 = sim(genomes["EC590"][1][0][1], 6000)
    m1, m2 = a1 + b1 + c1, a2 + b2 + c2
    for i in range(300):
        j = int(rng.integers(0, len(m1)))
        m1.append(m1[j]); m2.append(m2[j])
    write_fastq(str(d / "s_1.fq"), m1)
    write_fastq(str(d / "s_2.fq"), m2)
    # every 8th pair: K12 at ~0.75x, EC590 at ~0.5x — median k-mer coverage 1, so a lambda and an interval are estimated
    write_fastq(str(d / "thin_1.fq"), m1[::8])
    write_fastq(str(d / "thin_2.fq"), m2[::8])
    p = run("sketch", *[genomes[n][0] for n in ("EC590", "K12", "O157", "rand")], "-c", "50", "-o", d / "db")
    assert p.returncode == 0, p.stderr[-3000:]
    return dict(dir=d, db=d / "db.syldb")


@pytest.fixture(scope="module")
def data(tmp_path_factory, golden_dir):
    return build_inputs(tmp_path_factory.mktemp("cli_bootstrap"), golden_dir)


def ci_columns(stdout, command):
    rows = [line.split("\t") for line in stdout.splitlines()[1:]]
    at = (6, 8) if command == "profile" else (4, 6)               # ANI_5-95_percentile, Lambda_5-95_percentile
    return [(r[at[0]], r[at[1]]) for r in rows]


@pytest.mark.parametrize("command", ["profile", "query"])
def test_device_intervals_are_the_hosts_bytes(data, command):
    d = data["dir"]
    rows_with_ci = 0
    for reads in ("s", "thin"):
        args = (command, data["db"], "-c", "50", "-1", d / f"{reads}_1.fq", "-2", d / f"{reads}_2.fq")
        dev, host = run(*args, bootstrap="only"), run(*args, bootstrap="0")
        assert dev.returncode == 0, dev.stderr[-3000:]
        assert host.returncode == 0, host.stderr[-3000:]
        assert dev.stdout == host.stdout and len(host.stdout.splitlines()) >= 2
        rows_with_ci += sum(1 for a, l in ci_columns(host.stdout, command) if a != "NA-NA" and l != "NA-NA")
        if reads == "s":
            continue
        assert run(*args).stdout == host.stdout                    # the default route
        no_ci = [run(*args, "--no-ci", bootstrap=b) for b in ("only", "0")]
        assert no_ci[0].returncode == 0 and no_ci[0].stdout == no_ci[1].stdout
        assert all(c == ("NA-NA", "NA-NA") for c in ci_columns(no_ci[0].stdout, command))
        # --no-ci changes nothing but the two interval columns
        strip = lambda out: [[c for i, c in enumerate(line.split("\t")) if i not in ((6, 8) if command == "profile" else (4, 6))] for line in out.splitlines()]
        assert strip(no_ci[0].stdout) == strip(host.stdout)
    assert rows_with_ci >= 1


def test_a_bad_route_value_is_an_error(data):
    d = data["dir"]
    p = run("query", data["db"], "-c", "50", "-1", d / "thin_1.fq", "-2", d / "thin_2.fq", bootstrap="maybe")
    assert p.returncode == 1 and "SYLPH_HIP_BOOTSTRAP_DEVICE" in p.stderr
