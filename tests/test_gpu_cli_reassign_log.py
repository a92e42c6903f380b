"""GPU tests of `sylph-hip profile --log-reassignments`: the log on stderr against the oracle's sketches and statistics and a direct
restatement of winner_table's edge count (contain.rs:410-456) and of the line get_stats prints for a genome that falls below the
ANI cut only after the reassignment (contain.rs:749-761); the TSV untouched by the flag; `query` ignoring it."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

from .helpers import ACGT, random_seq, revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sylph_amd", "sylph-hip")
ORDER = ("EC590", "K12", "O157", "rand", "K12w")
HEADER = "------------- Logging k-mer reassignments -----------------"
PREFIX = "INFO  [sylph_hip] "


def run(*args):
    env = dict(os.environ, SYLPH_HIP_EXACT_DEDUP="1")                  # the oracle's pair set is the exact one
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    return p


def write_fasta(path, records, width=70):
    with open(path, "wb") as f:
        for name, seq in records:
            f.write(b">" + name + b"\n")
            s = bytes(seq)
            for i in range(0, len(s), width):
                f.write(s[i:i + width] + b"\n")


def write_fastq(path, reads):
    with open(path, "wb") as f:
        for i, s in enumerate(reads):
            f.write(b"@r" + str(i).encode() + b"\n" + bytes(s) + b"\n+\n" + b"I" * len(s) + b"\n")


def make_data(d, golden_dir):
    """The three E. coli slices + a random genome, and paired reads from K12 (6x) and EC590 (4x).  The slices are different
    regions of their genomes and share one k-mer at most, so the strain that loses k-mers is constructed: "K12w" = the first 95 %
    of the K12 slice with 0.3 % of its bases changed + 15 kb of its own, sequenced at 3x.  It passes the first pass on the k-mers
    it shares with K12, loses them all to K12 (the higher ANI) — an edge of a thousand k-mers — and falls below the ANI cut on
    what is left: the seventh of its k-mers that is its own (0.14^(1/31) = 0.94)."""
    z = np.load(os.path.join(golden_dir, "ecoli_slices.npz"))
    rng = np.random.default_rng(321)
    genomes = {}
    for gi, name in enumerate(("EC590", "K12", "O157")):
        b, off = z[f"g{gi}_bases"], z[f"g{gi}_off"]
        recs = [(f"{name}_contig{i} test genome".encode(), b[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]
        genomes[name] = (os.path.join(d, f"{name}.fasta"), recs)
    genomes["rand"] = (os.path.join(d, "rand.fa"), [(b"random_genome", random_seq(rng, 120000))])
    k12 = genomes["K12"][1][0][1]
    strain = k12[:len(k12) * 95 // 100].copy()
    at = rng.random(len(strain)) < 0.003
    strain[at] = rng.choice(ACGT, size=int(at.sum()))
    genomes["K12w"] = (os.path.join(d, "K12w.fa"), [(b"K12w_contig0 constructed strain", np.concatenate([strain, random_seq(rng, 15000)]))])
    for path, recs in genomes.values():
        write_fasta(path, recs)

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
            m1.append(a)
            m2.append(b)
        return m1, m2
    m1, m2 = [], []
    for name, cov in (("K12", 6.0), ("EC590", 4.0), ("K12w", 3.0)):
        for _, seq in genomes[name][1]:
            a, b = sim(seq, int(cov * len(seq) / 200))
            m1 += a
            m2 += b
    write_fastq(os.path.join(d, "s_1.fq"), m1)
    write_fastq(os.path.join(d, "s_2.fq"), m2)
    return dict(dir=d, genomes=genomes, m1=m1, m2=m2)


def oracle_log(data):
    """-> (index lines, edge lines, 'after reassigning' lines) as the reference would log them for the fixture's one sample: the
    oracle's sketches and statistics as in tests/test_gpu_cli.py's expected_rows, the winner table and the edges with dictionaries"""
    gs = []
    for name in ORDER:
        path, recs = data["genomes"][name]
        b, off = O.concat([bytes(r[1]) for r in recs])
        g = O.sketch_genome(b, off)
        gs.append(dict(path=path, contig=recs[0][0].decode(), kmers=g["genome_kmers"], tracked=g["tracked"]))
    b, off = O.concat([bytes(x) for p in zip(data["m1"], data["m2"]) for x in p])
    s = O.sketch_reads(b, off, paired=True)
    db = np.concatenate([g["kmers"] for g in gs])
    goff = np.zeros(len(gs) + 1, dtype=np.uint64)
    goff[1:] = np.cumsum([len(g["kmers"]) for g in gs])
    cc, covs, _ = O.contain(s["kmers"], s["counts"], db, goff)
    res = []                                                           # the passing list, in genome order
    for i, g in enumerate(gs):
        if cc[i]:
            st = O.stats(covs[i], len(g["kmers"]), min_ani=0.95)
            if st.passed:
                res.append((i, st.final_est_ani))
    index = [f"Index\t{r}\t{gs[i]['path']}\t{gs[i]['contig']}" for r, (i, _) in enumerate(res)]
    winner = {}                                                        # contain.rs:410-430
    for r, (i, ani) in enumerate(res):
        for km in gs[i]["kmers"].tolist() + gs[i]["tracked"].tolist():
            if km not in winner or ani > winner[km][0]:
                winner[km] = (ani, r)
    edges = {}                                                         # :440-449
    for r, (i, _) in enumerate(res):
        for km in gs[i]["kmers"].tolist():
            if winner[km][1] != r:
                edges[(r, winner[km][1])] = edges.get((r, winner[km][1]), 0) + 1
    edge_lines = [f"{w}->{l}\t{c}\tkmers reassigned" for (l, w), c in sorted(edges.items()) if c > 10]
    smap = dict(zip(s["kmers"].tolist(), s["counts"].tolist()))
    dropped = []                                                       # :749-761, the second get_stats pass
    for r, (i, _) in enumerate(res):
        cv = [smap[km] for km in gs[i]["kmers"].tolist() if smap.get(km, 0) and winner[km][1] == r]
        lost = sum(1 for km in gs[i]["kmers"].tolist() if smap.get(km, 0) and winner[km][1] != r)
        if not cv:
            continue
        st = O.stats(np.array(cv, dtype=np.uint32), len(gs[i]["kmers"]), min_ani=0.95)
        if not st.passed:
            dropped.append(f"Genome/contig {gs[i]['path']}/{gs[i]['contig']} has ANI = {st.final_est_ani * 100:.2f} < 95.00 after reassigning "
                           f"{lost} k-mers ({len(cv)} contained k-mers after reassign)")
    return index, edge_lines, dropped


@pytest.fixture(scope="module")
def data(tmp_path_factory, golden_dir):
    d = make_data(str(tmp_path_factory.mktemp("cli_reassign_log")), golden_dir)
    out = os.path.join(d["dir"], "out")
    run("sketch", *[d["genomes"][n][0] for n in ORDER], "-o", os.path.join(out, "db"), "-d", out, "-1", os.path.join(d["dir"], "s_1.fq"), "-2",
        os.path.join(d["dir"], "s_2.fq"))
    d["db"], d["sample"] = os.path.join(out, "db.syldb"), os.path.join(out, "s_1.fq.paired.sylsp")
    d["log"] = oracle_log(d)
    d["plain"] = run("profile", d["db"], d["sample"])
    d["logged"] = run("profile", d["db"], d["sample"], "--log-reassignments")
    return d


def info_lines(stderr):
    return [l[len(PREFIX):] for l in stderr.split("\n") if l.startswith(PREFIX)]


LOG_LINE = re.compile(r"^(Index\t|\d+->\d+\t|Genome/contig .* after reassigning )|Logging k-mer reassignments")


def test_log_holds_the_index_and_the_oracles_edges(data):
    index, edges, _ = data["log"]
    assert len(index) >= 3 and len(edges) >= 1                          # the fixture really has an edge above 10 k-mers
    lines = info_lines(data["logged"].stderr)
    at = lines.index(HEADER)
    assert lines.count(HEADER) == 1
    assert lines[at + 1:at + 1 + len(index)] == index                   # every passing genome, in result order, file and first contig
    got_edges = [l for l in lines if re.match(r"^\d+->\d+\t", l)]
    assert got_edges == edges                                           # exactly the oracle's, in (loser, winner) order
    assert lines[at + 1 + len(index):at + 1 + len(index) + len(edges)] == edges   # and the block is contiguous


def test_tsv_is_untouched_and_nothing_is_logged_without_the_flag(data):
    assert data["logged"].stdout == data["plain"].stdout and len(data["plain"].stdout.strip().split("\n")) >= 3
    assert not [l for l in info_lines(data["plain"].stderr) if LOG_LINE.search(l)]


def test_query_ignores_the_flag(data):
    q = run("query", data["db"], data["sample"], "--log-reassignments")
    assert q.stdout == run("query", data["db"], data["sample"]).stdout and len(q.stdout.strip().split("\n")) >= 3
    assert not [l for l in info_lines(q.stderr) if LOG_LINE.search(l)]


def test_genome_dropped_by_the_reassignment_is_named(data):
    _, _, dropped = data["log"]
    assert len(dropped) >= 1                                            # the constructed strain
    got = [l for l in info_lines(data["logged"].stderr) if l.startswith("Genome/contig ")]
    assert got == dropped


def test_raw_reads_through_the_pipeline_log_the_same(data):
    """a raw sample comes out of the pipeline with its table in device memory and is reported against the replica it ran on: same
    log, same rows as the sketched sample"""
    d = data["dir"]
    p = run("profile", data["db"], "-1", os.path.join(d, "s_1.fq"), "-2", os.path.join(d, "s_2.fq"), "--log-reassignments")
    assert [l for l in info_lines(p.stderr) if LOG_LINE.search(l)] == [l for l in info_lines(data["logged"].stderr) if LOG_LINE.search(l)]
    assert p.stdout == data["plain"].stdout
