"""GPU tests of the genome files' device road through the `sylph-hip` command (host/cmd_sketch.cpp GenomeBatch::add_window_device over
csrc/fasta.hip): a database built from plain, gzip and bzip2 FASTA files — among them a FASTQ-format genome, a file that is not FASTA
and a FASTA with a '\\r' inside a line, which the device declines and the host reader takes — must be the database of the host road
(SYLPH_HIP_FASTA_DEVICE=0, and unset: the device road is opt-in, SYLPH_HIP_FASTA_DEVICE=1), byte for byte, with the same warnings, for every -t, with and without -i, through -g, -l and --gl; the
trace must show that ONLY the three odd files were declined; and `profile` with raw genome files gives the same TSV on both roads."""
import bz2
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from .fasta_texts import fasta_text

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sylph_amd", "sylph-hip")
TRACE = re.compile(r"^\[sylph_hip feed\] genomes fasta-device files=(\d+) declined=(\d+)\s+[\d.]+ ms$")


def run(args, cwd, road, trace=False):
    env = dict(os.environ, SYLPH_HIP_EXACT_DEDUP="1")
    env.pop("SYLPH_HIP_FASTA_DEVICE", None)
    env.pop("SYLPH_HIP_FEED_TRACE", None)
    if road is not None:
        env["SYLPH_HIP_FASTA_DEVICE"] = road
    if trace:
        env["SYLPH_HIP_FEED_TRACE"] = "1"
    os.makedirs(cwd, exist_ok=True)
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=env, cwd=str(cwd))
    assert p.returncode == 0, p.stderr[-3000:]
    return p


def messages(stderr):
    """the command's own messages: everything but the trace's lines and the timing notes"""
    return [ln for ln in stderr.splitlines() if not ln.startswith("[sylph_hip") and "timing:" not in ln]


def road_counts(stderr):
    files = declined = 0
    for ln in stderr.splitlines():
        m = TRACE.match(ln)
        if m:
            files += int(m.group(1))
            declined += int(m.group(2))
    return files, declined


@pytest.fixture(scope="module")
def genomes(tmp_path_factory, golden_dir):
    d = tmp_path_factory.mktemp("cli_fasta")
    z = np.load(os.path.join(golden_dir, "ecoli_slices.npz"))
    good, texts = [], {}
    for gi, name in enumerate(("EC590", "K12", "O157")):
        b = z[f"g{gi}_bases"].tobytes()
        cuts = [0, 40, 40, len(b) // 5, len(b) // 2, len(b) // 2 + 1000, len(b)]       # contigs: 40 bases, none, and four long ones
        recs = [b[cuts[i]:cuts[i + 1]] for i in range(len(cuts) - 1)]
        ids = [b"%s_contig%d some > @ description" % (name.encode(), i) for i in range(len(recs))]
        text = fasta_text(recs, ids, width=(70, 60, 0)[gi], eol=(b"\n", b"\r\n", b"\n")[gi], last_eol=gi != 2, blank_every=(0, 9, 0)[gi])
        texts[name] = text
        for suffix, data in ((".fa", text), (".fa.gz", gzip.compress(text, 6)), (".bz2.fa", bz2.compress(text))):
            p = str(d / (name + suffix))
            with open(p, "wb") as f:
                f.write(data)
            good.append(p)
    k12 = z["g1_bases"].tobytes()
    odd = {"fastq_format.fa": b"".join(b"@r%d\n%s\n+\n%s\n" % (i, k12[i * 5000:i * 5000 + 5000], b"I" * 5000) for i in range(8)),
           "not_fasta.fa": b"this is\nnot a sequence file\n",
           "cr_inside.fa": b">cr inside a line\n" + k12[:3000] + b"\r" + k12[3000:9000] + b"\n" + k12[9000:30000] + b"\n"}
    odd_paths = []
    for name, data in odd.items():
        p = str(d / name)
        with open(p, "wb") as f:
            f.write(data)
        odd_paths.append(p)
    # the odd files between the good ones, so that the road changes in the middle of a window
    files = good[:2] + odd_paths[:1] + good[2:5] + odd_paths[1:2] + good[5:8] + odd_paths[2:] + good[8:]
    return dict(dir=d, files=files, n_good=len(good), n_odd=len(odd_paths), k12=k12)


@pytest.mark.parametrize("t,ind,how", [("1", False, "-g"), ("1", True, "-g"), ("4", False, "-g"), ("4", True, "-g"), ("4", False, "-l"), ("1", True, "--gl")])
def test_database_is_the_host_roads_database(genomes, t, ind, how):
    d, files = genomes["dir"], genomes["files"]
    with open(d / "all.list", "w") as f:
        f.write("\n".join(files) + "\n")
    n = f"{t}{int(ind)}{how.strip('-')}"
    args = ["sketch", "-t", t, "-c", "100", "-o", "db"] + (["-i"] if ind else []) + ([how] + files if how == "-g" else [how, d / "all.list"])
    host = run(args, d / f"host{n}", "0" if t == "1" else None, trace=True)      # (unset: the host road)
    dev = run(args, d / f"dev{n}", "1", trace=True)
    a, b = open(d / f"host{n}" / "db.syldb", "rb").read(), open(d / f"dev{n}" / "db.syldb", "rb").read()
    assert len(a) > 10000 and a == b
    assert messages(host.stderr) == messages(dev.stderr)
    assert sum("not a valid fasta/fastq file" in ln for ln in messages(dev.stderr)) == 1
    assert road_counts(host.stderr) == (0, 0)
    n_files, n_declined = road_counts(dev.stderr)
    assert n_files == len(files) and n_declined == genomes["n_odd"], dev.stderr[-2000:]


def test_profile_with_raw_genome_files(genomes):
    d, files, k12 = genomes["dir"], genomes["files"], genomes["k12"]
    rng = np.random.default_rng(5)
    with open(d / "reads.fq", "wb") as f:
        for i, s in enumerate(rng.integers(0, len(k12) - 150, size=6000)):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, k12[int(s):int(s) + 150], b"I" * 150))
    args = ["profile", "-t", "3", "-c", "100", d / "reads.fq"] + files
    host = run(args, d / "p_host", "0")
    dev = run(args, d / "p_dev", "1", trace=True)
    assert len(host.stdout.splitlines()) >= 2 and host.stdout == dev.stdout
    assert road_counts(dev.stderr) == (len(files), genomes["n_odd"])
