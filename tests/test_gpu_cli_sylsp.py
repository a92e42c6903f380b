"""GPU tests of `sylph-hip profile` / `query` over sketch files (*.sylsp) on the device's road — the files' tables unpacked on the GPU
and sent through the pipeline (SYLPH_HIP_SYLSP_DEVICE=1) — against the host's road (=0) on the same files: the same bytes on stdout
and in the -o file, the same messages, order and exit status when a file is refused or broken.  Half the files are as
`sylph-hip sketch` wrote them (ascending), half rewritten with shuffled entries and a few repeated keys."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from .helpers import random_seq
from .sylsp_tables import ENTRY
from .test_gpu_cli_reassign_log import write_fasta, write_fastq

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sylph_amd", "sylph-hip")
N_SAMPLES = 8
TRACE = re.compile(r"^\[sylph_hip feed\] sylsp (\S+): route (\w+), table ([a-z ]+), (\d+) entries -> (\d+) k-mers$")


def run(road, *args, check=True, **env):
    e = dict(os.environ, SYLPH_HIP_SYLSP_DEVICE=str(road), **env)
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=e)
    if check:
        assert p.returncode == 0, p.stderr[-3000:]
    return p


def rewrite_shuffled(src, dst, rng):
    """The same sketch in another entry order (standing in for hashbrown's), some keys repeated: copies with other counts in FRONT of
    the shuffled entries (the map keeps the later, original count) and one repeat BEHIND them (its count replaces the original)."""
    blob = open(src, "rb").read()
    n = struct.unpack_from("<Q", blob, 0)[0]
    entries = np.frombuffer(blob, dtype=ENTRY, count=n, offset=8)
    tail = blob[8 + 12 * n:]
    front = entries[rng.choice(n, size=5, replace=False)].copy()
    front["count"] += 100
    back = entries[rng.integers(0, n, size=1)].copy()
    back["count"] += 1
    out = np.concatenate([front, entries[rng.permutation(n)], back])
    assert not (out["kmer"][1:] > out["kmer"][:-1]).all()
    with open(dst, "wb") as f:
        f.write(struct.pack("<Q", len(out)) + out.tobytes() + tail)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cli_sylsp"))
    rng = np.random.default_rng(77)
    genomes = [random_seq(rng, 60000) for _ in range(5)]
    fastas = []
    for i, g in enumerate(genomes):
        fastas.append(os.path.join(d, f"g{i}.fa"))
        write_fasta(fastas[-1], [(f"genome{i}_contig".encode(), g)])
    fastqs = []
    for i in range(N_SAMPLES):
        reads = []
        for g, cov in ((genomes[i % 5], 4.0), (genomes[(i + 2) % 5], 2.0 + i % 3)):
            for s in rng.integers(0, len(g) - 150, size=int(cov * len(g) / 150)):
                r = g[s:s + 150].copy()
                e = rng.random(150) < 0.005
                r[e] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(e.sum()))
                reads.append(r)
        fastqs.append(os.path.join(d, f"s{i}.fq"))
        write_fastq(fastqs[-1], reads)
    out = os.path.join(d, "out")
    run(0, "sketch", *fastas, "-o", os.path.join(out, "db"), "-d", out, "-r", *fastqs[:N_SAMPLES])
    written = [os.path.join(out, f"s{i}.fq.sylsp") for i in range(N_SAMPLES)]
    samples, ascending = [], []
    for i, p in enumerate(written):
        assert os.path.exists(p)
        if i % 2:
            q = os.path.join(d, f"shuffled{i}.sylsp")
            rewrite_shuffled(p, q, rng)
            samples.append(q)
        else:
            samples.append(p)
        ascending.append(i % 2 == 0)
    big_c = os.path.join(d, "c400.sylsp")                                                      # a sketch the database's c = 200 cannot serve
    truncated = os.path.join(d, "truncated.sylsp")
    blob = open(written[2], "rb").read()
    n = struct.unpack_from("<Q", blob, 0)[0]
    assert struct.unpack_from("<Q", blob, 8 + 12 * n)[0] == 200                                # the tail starts with c
    with open(big_c, "wb") as f:
        f.write(blob[:8 + 12 * n] + struct.pack("<Q", 400) + blob[8 + 12 * n + 8:])
    with open(truncated, "wb") as f:
        f.write(blob[:8 + 12 * 100 + 7])
    host = {cmd: run(0, cmd, os.path.join(out, "db.syldb"), *samples) for cmd in ("profile", "query")}
    for cmd in host:
        assert len(host[cmd].stdout.strip().split("\n")) >= 1 + 2 * N_SAMPLES                  # two genomes per sample at the least
    return dict(dir=d, db=os.path.join(out, "db.syldb"), samples=samples, ascending=ascending, big_c=big_c, truncated=truncated, host=host)


@pytest.mark.parametrize("cmd", ["profile", "query"])
def test_device_road_prints_the_host_roads_bytes_and_names_its_route(data, cmd):
    o = os.path.join(data["dir"], f"{cmd}_device.tsv")
    p = run(1, cmd, data["db"], *data["samples"], SYLPH_HIP_FEED_TRACE="1")
    assert p.stdout == data["host"][cmd].stdout
    q = run(1, cmd, data["db"], *data["samples"], "-o", o)
    assert q.stdout == "" and open(o).read() == data["host"][cmd].stdout
    traced = [TRACE.match(l) for l in p.stderr.split("\n") if l.startswith("[sylph_hip feed] sylsp ")]
    assert all(traced) and [m.group(1) for m in traced] == data["samples"]                     # one line per sample, in input order
    for m, asc in zip(traced, data["ascending"]):
        assert m.group(2) == "device" and m.group(3) == ("ascending" if asc else "sorted on the device")
        assert int(m.group(5)) == int(m.group(4)) - (0 if asc else 6)                          # the six repeats are gone
    h = run(0, cmd, data["db"], *data["samples"][:2], SYLPH_HIP_FEED_TRACE="1")                # the host's road says so too
    assert [TRACE.match(l).group(2) for l in h.stderr.split("\n") if l.startswith("[sylph_hip feed] sylsp ")] == ["host", "host"]


@pytest.mark.parametrize("cmd", ["profile", "query"])
def test_estimate_unknown_walks_the_same_counts(data, cmd):
    a = run(1, cmd, data["db"], *data["samples"], "-u")
    b = run(0, cmd, data["db"], *data["samples"], "-u")
    assert a.stdout == b.stdout and len(a.stdout.strip().split("\n")) >= 1 + 2 * N_SAMPLES
    if cmd == "profile":
        assert a.stdout != data["host"][cmd].stdout                                            # (True_cov instead of Eff_cov in the header alone)


def test_two_replicas_sharing_the_gpu(data):
    p = run(1, "profile", data["db"], *data["samples"], "--gpus", 2, SYLPH_HIP_SHARE_GPUS="1")
    assert p.stdout == data["host"]["profile"].stdout
    assert "database replicated on 2 GPUs" in p.stderr


def test_log_reassignments_from_the_device_table(data):
    a = run(1, "profile", data["db"], *data["samples"], "--log-reassignments")
    b = run(0, "profile", data["db"], *data["samples"], "--log-reassignments")
    assert a.stdout == b.stdout == data["host"]["profile"].stdout

    def log(p):
        return [l for l in p.stderr.split("\n") if re.search(r"Logging k-mer reassignments|\] Index\t|\] \d+->\d+\t| after reassigning ", l)]
    assert log(a) == log(b) and len(log(a)) >= 3 * N_SAMPLES


def test_refused_and_broken_files_fail_as_on_the_host_road(data):
    """A sketch whose c the database cannot serve is named and skipped; a truncated one in the middle of the list ends the command
    when its turn comes — behind the rows of the files before it, with the host road's message and exit status."""
    s = data["samples"]
    files = [s[0], data["big_c"], s[1], s[2], data["truncated"], s[3], s[4]]
    a = run(1, "profile", data["db"], *files, check=False)
    b = run(0, "profile", data["db"], *files, check=False)

    def told(p):
        return [l for l in p.stderr.split("\n") if l.startswith("ERROR") or "Finished sample" in l or "not a valid sketch" in l]
    assert a.returncode == b.returncode != 0
    assert told(a) == told(b)
    assert a.stdout == b.stdout
    names = {l.split("\t")[0] for l in a.stdout.strip().split("\n")[1:]}
    assert len(names) == 3                                                                     # the three good files in front of the broken one
    assert any("value of -c is 400" in l for l in told(a)) and any("truncated.sylsp` is not a valid sketch" in l for l in told(a))
    assert sum("Finished sample" in l for l in told(a)) == 4                                   # (the refused file "finishes" too, as in the reference)


def test_a_broken_file_fails_the_command_at_its_turn(data):
    """The failure rule of the command's hand-over (host/ordered_ahead.hpp), end to end with the rows summarised on the device: of three
    files with the middle one truncated, the rows of the first are out — all of them, nothing of the third — and the command fails."""
    s = data["samples"]
    alone = run(1, "profile", data["db"], s[0], SYLPH_HIP_STATS_DEVICE="1")
    assert len(alone.stdout.strip().split("\n")) >= 1 + 2                                      # the header and two genomes at the least
    p = run(1, "profile", data["db"], s[0], data["truncated"], s[1], check=False, SYLPH_HIP_STATS_DEVICE="1")
    assert p.returncode != 0
    assert p.stdout == alone.stdout
