"""GPU tests of genome files that hold more than one device batch, through the `sylph-hip` command (host/cmd_sketch.cpp
GenomeBatch::append over csrc/genome_acc.hip).  SYLPH_HIP_GENOME_PUSH_BASES=50000 makes a 470 kb FASTA of 40 contigs such a file: as one
genome (`sketch -g`) its contigs go through the accumulator in several pushes, with -i its records are cut into several batches, and
either way the database must be the one written without the knob, byte for byte, on the device FASTA road and on the host road.  A
contig of 60 kb is then more than any batch holds: as part of one genome it refuses its file, as a record of its own only it is
skipped.  `profile` with the raw genome file gives the same TSV with and without the knob."""
import os
import re
import subprocess

import numpy as np
import pytest

from .fasta_texts import fasta_text
from .helpers import random_seq, revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sylph_amd", "sylph-hip")
KNOB = "50000"
ACCUMULATE = re.compile(r"^\[sylph_hip feed\] genomes accumulate: (\S+) contigs=(\d+) bases=(\d+) pushes=(\d+) seeds=(\d+)\s+[\d.]+ ms$", re.M)
SPLIT = re.compile(r"^\[sylph_hip feed\] genomes split: (\S+) records=(\d+) batches=(\d+) skipped=(\d+)\s+[\d.]+ ms$", re.M)
ROADS = ["1", "0"]                      # SYLPH_HIP_FASTA_DEVICE


def run(args, cwd, files, knob=None, road=None):
    """the command in a directory of its own that holds `files` (name -> bytes): the names in its output do not depend on the run"""
    env = dict(os.environ, SYLPH_HIP_EXACT_DEDUP="1", SYLPH_HIP_FEED_TRACE="1")
    for v in ("SYLPH_HIP_FASTA_DEVICE", "SYLPH_HIP_GENOME_PUSH_BASES"):
        env.pop(v, None)
    if road is not None:
        env["SYLPH_HIP_FASTA_DEVICE"] = road
    if knob is not None:
        env["SYLPH_HIP_GENOME_PUSH_BASES"] = knob
    os.makedirs(cwd, exist_ok=True)
    for name, data in files.items():
        with open(os.path.join(cwd, name), "wb") as f:
            f.write(data)
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=env, cwd=str(cwd))
    assert p.returncode == 0, p.stderr[-3000:]
    return p


def db_of(cwd):
    with open(os.path.join(cwd, "db.syldb"), "rb") as f:
        return f.read()


def messages(stderr):
    return [ln for ln in stderr.splitlines() if not ln.startswith("[sylph_hip") and "timing:" not in ln]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_big_genomes")
    rng = np.random.default_rng(20261021)
    lens = rng.integers(5000, 20001, size=40)
    recs = [random_seq(rng, int(n)) for n in lens]
    rep = recs[3][1000:3000].copy()                       # a repeat whose copies land in different pushes and different batches
    recs[20][2000:4000] = rep
    recs[35][500:2500] = revcomp(rep)
    ids = [b"main_contig%d len=%d" % (i, len(r)) for i, r in enumerate(recs)]
    main = fasta_text([r.tobytes() for r in recs], ids, width=80)
    big_recs = [random_seq(rng, n).tobytes() for n in (8000, 60000, 9000)]
    big_ids = [b"small_before", b"oversize_contig 60 kb", b"small_after"]
    big = fasta_text(big_recs, big_ids, width=70)
    big_without = fasta_text([big_recs[0], big_recs[2]], [big_ids[0], big_ids[2]], width=70)
    genome = np.concatenate(recs)
    reads = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, genome[int(s):int(s) + 150].tobytes(), b"I" * 150)
                     for i, s in enumerate(rng.integers(0, len(genome) - 150, size=4000)))
    files = {"main.fa": main, "big.fa": big, "reads.fq": reads}
    # what the command writes without the knob (the default road)
    base = dict(sketch=["sketch", "-t", "2", "-c", "100", "-o", "db"])
    run(base["sketch"] + ["-g", "main.fa"], d / "ref_g", files)
    run(base["sketch"] + ["-i", "-g", "main.fa"], d / "ref_i", files)
    run(base["sketch"] + ["-i", "-g", "main.fa", "big.fa"], d / "ref_i_without", dict(files, **{"big.fa": big_without}))
    prof = run(["profile", "-t", "2", "-c", "100", "reads.fq", "main.fa"], d / "ref_profile", files)
    assert len(prof.stdout.splitlines()) >= 2
    return dict(dir=d, files=files, sketch=base["sketch"], n_bases=int(sum(lens)), ref_g=db_of(d / "ref_g"), ref_i=db_of(d / "ref_i"),
                ref_i_without=db_of(d / "ref_i_without"), ref_profile=prof.stdout)


@pytest.mark.parametrize("road", ROADS)
def test_one_genome_goes_through_the_accumulator(inputs, road):
    d = inputs["dir"] / f"g_{road}"
    p = run(inputs["sketch"] + ["-g", "main.fa"], d, inputs["files"], knob=KNOB, road=road)
    assert len(inputs["ref_g"]) > 10000 and db_of(d) == inputs["ref_g"]
    m = ACCUMULATE.findall(p.stderr)
    assert len(m) == 1 and not SPLIT.findall(p.stderr), p.stderr[-2000:]
    name, contigs, bases, pushes, seeds = m[0]
    assert name == "main.fa" and int(contigs) == 40 and int(bases) == inputs["n_bases"] and int(pushes) >= 3 and int(seeds) > 1000
    assert not any("skipping" in ln for ln in messages(p.stderr))


@pytest.mark.parametrize("road", ROADS)
def test_records_are_split_into_batches(inputs, road):
    d = inputs["dir"] / f"i_{road}"
    p = run(inputs["sketch"] + ["-i", "-g", "main.fa"], d, inputs["files"], knob=KNOB, road=road)
    assert len(inputs["ref_i"]) > 10000 and db_of(d) == inputs["ref_i"]
    m = SPLIT.findall(p.stderr)
    assert len(m) == 1 and not ACCUMULATE.findall(p.stderr), p.stderr[-2000:]
    name, records, batches, skipped = m[0]
    assert name == "main.fa" and int(records) == 40 and int(batches) >= 3 and int(skipped) == 0


@pytest.mark.parametrize("road", ROADS)
def test_oversize_contig_refuses_its_genome_only(inputs, road):
    d = inputs["dir"] / f"g_over_{road}"
    p = run(inputs["sketch"] + ["-g", "main.fa", "big.fa"], d, inputs["files"], knob=KNOB, road=road)
    assert db_of(d) == inputs["ref_g"]                      # the first file's genome is there, the second file's is not
    warned = [ln for ln in messages(p.stderr) if "skipping" in ln]
    assert len(warned) == 1 and "big.fa" in warned[0] and "oversize_contig" in warned[0] and "60000 bases" in warned[0], p.stderr[-2000:]
    assert [m[0] for m in ACCUMULATE.findall(p.stderr)] == ["main.fa"]


@pytest.mark.parametrize("road", ROADS)
def test_oversize_record_alone_is_skipped(inputs, road):
    d = inputs["dir"] / f"i_over_{road}"
    p = run(inputs["sketch"] + ["-i", "-g", "main.fa", "big.fa"], d, inputs["files"], knob=KNOB, road=road)
    assert db_of(d) == inputs["ref_i_without"] and len(inputs["ref_i_without"]) > len(inputs["ref_i"])
    warned = [ln for ln in messages(p.stderr) if "skipping" in ln]
    assert len(warned) == 1 and "big.fa" in warned[0] and "oversize_contig" in warned[0] and "60000 bases" in warned[0], p.stderr[-2000:]
    m = {name: (int(records), int(batches), int(skipped)) for name, records, batches, skipped in SPLIT.findall(p.stderr)}
    assert m["big.fa"] == (3, 2, 1) and m["main.fa"][0] == 40 and m["main.fa"][2] == 0


@pytest.mark.parametrize("road", ROADS)
def test_profile_with_the_raw_genome_file(inputs, road):
    d = inputs["dir"] / f"profile_{road}"
    p = run(["profile", "-t", "2", "-c", "100", "reads.fq", "main.fa"], d, inputs["files"], knob=KNOB, road=road)
    assert p.stdout == inputs["ref_profile"]
    m = ACCUMULATE.findall(p.stderr)
    assert len(m) == 1 and int(m[0][3]) >= 3, p.stderr[-2000:]
