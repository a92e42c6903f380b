"""`sylph-hip` on INTERLEAVED paired reads (--interleaved F, --lI, --no-mate-check): F means `-1 A -2 B` with A = the even records of
F and B = the odd ones, on every road a sample's reads can take — plain text (the indexed host feed for a command's first sample, the
device route behind it), gzip and bzip2 decoded on the device whole and streamed, FASTA, the host feed alone and the sequential
reader.  The k-mer table, `paired`, c, k and mean_read_length of the .sylsp must be those of the two-file sample; `profile` and `query`
must print the two-file command's rows; a file that lost a read is skipped with one warning that names both ids, on every road."""
import bz2
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from .helpers import random_seq, revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sylph_amd", "sylph-hip")
N_PAIRS = 4000
LOST = 1777                                       # the pair at which bad.* lost its mate 2
PUSHED = "device route: interleaved pairs pushed"
ENV_NAMES = ("SYLPH_HIP_INFLATE_STREAM", "SYLPH_HIP_INFLATE_WHOLE_MAX", "SYLPH_HIP_INFLATE_SLICE", "SYLPH_HIP_BUNZIP2_STREAM", "SYLPH_HIP_BUNZIP2_WHOLE_MAX",
             "SYLPH_HIP_BUNZIP2_SLICE", "SYLPH_HIP_FEED_DEVICE", "SYLPH_HIP_SEQUENTIAL_FEED", "SYLPH_HIP_INFLATE_DEVICE", "SYLPH_HIP_BUNZIP2_DEVICE",
             "SYLPH_HIP_FASTA_READS_DEVICE", "SYLPH_HIP_EXACT_DEDUP")
# road -> (the file of il/, environment, what the feed trace must say, what it must not say)
ROADS = {
    "plain_host_feed_then_device": ("s.fq", {}, ["host feed: interleaved mates checked", PUSHED], []),
    "gzip": ("s.fq.gz", {}, ["device route: gzip inflated on the device", "device route: interleaved mates checked", PUSHED], ["stream route"]),
    "bzip2": ("s.fq.bz2", {}, ["device route: bzip2 decoded on the device", PUSHED], ["stream route"]),
    "gzip_streamed": ("s.fq.gz", dict(SYLPH_HIP_INFLATE_WHOLE_MAX=str(256 << 10), SYLPH_HIP_INFLATE_SLICE=str(64 << 10)),
                      ["interleaved gzip streamed", "interleaved pairs of FASTQ records"], [PUSHED]),
    "bzip2_streamed": ("s.fq.bz2", dict(SYLPH_HIP_BUNZIP2_WHOLE_MAX=str(128 << 10), SYLPH_HIP_BUNZIP2_SLICE=str(64 << 10)),
                       ["interleaved bzip2 streamed", "interleaved pairs of FASTQ records"], [PUSHED]),
    "fasta": ("s.fa", {}, ["device route: FASTA records found", PUSHED], []),
    "fasta_gzip_streamed": ("s.fa.gz", dict(SYLPH_HIP_INFLATE_WHOLE_MAX=str(128 << 10), SYLPH_HIP_INFLATE_SLICE=str(64 << 10)),
                            ["interleaved gzip streamed", "interleaved pairs of FASTA records"], [PUSHED]),
    "host_feed": ("s.fq", dict(SYLPH_HIP_FEED_DEVICE="0"), ["host feed: interleaved mates checked"], ["device route"]),
    "sequential": ("s.fq", dict(SYLPH_HIP_SEQUENTIAL_FEED="1"), ["sequential reader: interleaved"], ["device route", "host feed:"]),
    "sequential_fasta_gzip": ("s.fa.gz", dict(SYLPH_HIP_SEQUENTIAL_FEED="1"), ["sequential reader: interleaved"], ["device route"]),
}


def records(rng, genome, n):
    """n pairs: (header 1, sequence 1, header 2, sequence 2), Illumina-style names whose ids are equal, every fifth pair /1 and /2"""
    out = []
    for i in range(n):
        la, lb = int(rng.integers(100, 151)), int(rng.integers(100, 151))
        s = int(rng.integers(0, len(genome) - 500))
        a, b = genome[s:s + la], revcomp(genome[s + 200:s + 200 + lb])
        ident = b"A00123:45:HXXXXXXXX:1:%d:%d:%d" % (1101 + i // 900, 1000 + (i * 37) % 30000, i)
        if i % 5 == 4:
            out.append((ident + b"/1", bytes(a), ident + b"/2", bytes(b)))
        else:
            out.append((ident + b" 1:N:0:ACGT", bytes(a), ident + b" 2:N:0:ACGT", bytes(b)))
    for i in range(50, n, 97):                                                           # whole pairs twice: the dedup has work
        out[i] = (out[i][0], out[i - 1][1], out[i][2], out[i - 1][3])
    return out


def fastq(recs):
    return b"".join(b"@" + h + b"\n" + s + b"\n+\n" + bytes([70 - (j % 13 == 0) * 12 for j in range(len(s))]) + b"\n" for h, s in recs)


def fasta(recs):
    return b"".join(b">" + h + b"\n" + s + b"\n" for h, s in recs)


def gz6(data):
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    return co.compress(data) + co.flush()


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """two/: the mates in two files; il/: the same pairs in one, under the names of ROADS, a copy (s2.fq), the file without its last
    record (odd.fq) and the file that lost one read (bad.*); lost/: that file's even and odd records in two files"""
    d = tmp_path_factory.mktemp("cli_interleaved")
    rng = np.random.default_rng(91)
    genome = random_seq(rng, 200000)
    pairs = records(rng, genome, N_PAIRS)
    a, b = [(p[0], p[1]) for p in pairs], [(p[2], p[3]) for p in pairs]
    f = [x for p in zip(a, b) for x in p]
    bad = f[:2 * LOST + 1] + f[2 * LOST + 2:]
    for sub in ("two", "il", "lost"):
        (d / sub).mkdir()
    (d / "two" / "s_1.fq").write_bytes(fastq(a))
    (d / "two" / "s_2.fq").write_bytes(fastq(b))
    (d / "two" / "short_2.fq").write_bytes(fastq(b[:-1]))
    (d / "lost" / "bad_1.fq").write_bytes(fastq(bad[0::2]))
    (d / "lost" / "bad_2.fq").write_bytes(fastq(bad[1::2]))
    for name, recs in (("s", f), ("bad", bad)):
        fq, fa = fastq(recs), fasta(recs)
        (d / "il" / f"{name}.fq").write_bytes(fq)
        (d / "il" / f"{name}.fa").write_bytes(fa)
        (d / "il" / f"{name}.fq.gz").write_bytes(gz6(fq))
        (d / "il" / f"{name}.fa.gz").write_bytes(gz6(fa))
        (d / "il" / f"{name}.fq.bz2").write_bytes(bz2.compress(fq, 1))
    assert len(gz6(fastq(f))) > (256 << 10) and len(gz6(fasta(f))) > (128 << 10) and len(bz2.compress(fastq(f), 1)) > (128 << 10)
    (d / "il" / "s2.fq").write_bytes(fastq(f))
    (d / "il" / "odd.fq").write_bytes(fastq(f[:-1]))
    with open(d / "genome.fa", "wb") as g:
        g.write(b">genome\n" + bytes(genome) + b"\n")
    ids = (bad[2 * LOST][0].split()[0].decode(), bad[2 * LOST + 1][0].split()[0].decode())
    return dict(dir=d, lost_ids=ids, want={})


def run(cwd, *args, env=None, check=True, exact=True):
    e = dict(os.environ, SYLPH_HIP_FEED_TRACE="1")
    for k in ENV_NAMES:
        e.pop(k, None)
    if exact:
        e["SYLPH_HIP_EXACT_DEDUP"] = "1"
    e.update(env or {})
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=e, cwd=str(cwd))
    if check:
        assert p.returncode == 0, p.stderr[-3000:]
    return p


def read_sylsp(path):
    """SequencesSketch (types.rs:145-155): the (u64, u32) table, c, k, file_name, Option<sample_name>, paired, mean_read_length"""
    raw = open(path, "rb").read()
    n = int.from_bytes(raw[:8], "little")
    t = np.frombuffer(raw, dtype=np.dtype([("k", "<u8"), ("c", "<u4")]), count=n, offset=8)
    o = 8 + 12 * n
    c, k, ln = struct.unpack_from("<QQQ", raw, o)
    o += 24
    name = raw[o:o + ln].decode()
    o += ln
    sample = None
    if raw[o]:
        (ls,) = struct.unpack_from("<Q", raw, o + 1)
        sample = raw[o + 9:o + 9 + ls].decode()
        o += 8 + ls
    o += 1
    paired = bool(raw[o])
    mean = raw[o + 1:o + 9]                                                              # the f64's bytes: compared bit for bit
    assert o + 9 == len(raw)
    order = np.argsort(t["k"], kind="stable")
    return dict(kmers=t["k"][order], counts=t["c"][order], c=c, k=k, file_name=name, sample_name=sample, paired=paired, mean=mean)


def assert_same_sample(got, want, tag):
    assert np.array_equal(got["kmers"], want["kmers"]) and np.array_equal(got["counts"], want["counts"]), tag
    assert (got["c"], got["k"], got["paired"], got["mean"]) == (want["c"], want["k"], True, want["mean"]), tag


def two_file(data, flags=(), exact=True, second="s_2.fq", first="s_1.fq", sub="two"):
    """the two-file sample's sketch, made once per set of flags"""
    key = (tuple(flags), exact, first, second)
    if key not in data["want"]:
        d = data["dir"]
        out = d / f"want_{len(data['want'])}"
        run(d / sub, "sketch", "-1", first, "-2", second, "-d", out, *flags, exact=exact)
        data["want"][key] = read_sylsp(out / f"{first}.paired.sylsp")
        assert len(data["want"][key]["kmers"]) > 500 and data["want"][key]["paired"]
    return data["want"][key]


@pytest.mark.parametrize("road", list(ROADS))
def test_every_road_gives_the_two_file_sample(data, road):
    d = data["dir"]
    name, env, says, says_not = ROADS[road]
    files = [name, "s2.fq"] if road.startswith("plain") else [name]                      # a command's first plain sample is fed by the host
    out = d / f"out_{road}"
    p = run(d / "il", "sketch", "-t", "1", "--interleaved", *files, "-d", out, env=env)
    for line in says:
        assert line in p.stderr, (line, p.stderr[-3000:])
    for line in says_not:
        assert line not in p.stderr, (line, p.stderr[-3000:])
    want = two_file(data)
    for f in files:
        got = read_sylsp(out / f"{f}.paired.sylsp")                                      # named as a pair is after its first file
        assert got["file_name"] == f and got["sample_name"] is None
        assert_same_sample(got, want, (road, f))


@pytest.mark.parametrize("flags,exact", [(("--fpr", "0"), False), ((), False), (("--no-dedup",), False), (("-c", "50", "-k", "21"), True)])
def test_dedup_rules_and_parameters_are_the_pairs(data, flags, exact):
    d = data["dir"]
    want = two_file(data, flags, exact)
    for name in ("s.fq.gz", "s.fa"):
        out = d / f"out_flags_{len(flags)}_{exact}_{name}"
        run(d / "il", "sketch", "--interleaved", name, "-d", out, *flags, exact=exact)
        assert_same_sample(read_sylsp(out / f"{name}.paired.sylsp"), want, (flags, name))


def test_a_last_record_without_a_mate_is_dropped(data):
    d = data["dir"]
    want = two_file(data, second="short_2.fq")                                           # the lock-step readers drop mate 1's surplus record
    assert not np.array_equal(want["kmers"], two_file(data)["kmers"]) or want["mean"] != two_file(data)["mean"]
    for env in ({}, dict(SYLPH_HIP_FEED_DEVICE="0"), dict(SYLPH_HIP_SEQUENTIAL_FEED="1")):
        out = d / f"out_odd_{len(env)}_{'_'.join(env)}"
        # (one sample thread: with the device feed on, the command's second plain sample takes the device route)
        run(d / "il", "sketch", "-t", "1", "--interleaved", "s2.fq", "odd.fq", "-d", out, env=env)
        assert_same_sample(read_sylsp(out / "odd.fq.paired.sylsp"), want, env)
        assert_same_sample(read_sylsp(out / "s2.fq.paired.sylsp"), two_file(data), env)


@pytest.mark.parametrize("road", list(ROADS))
def test_a_file_out_of_phase_is_skipped_on_every_road(data, road):
    d = data["dir"]
    name, env, _, _ = ROADS[road]
    bad = "bad" + name[1:]
    files = ["s2.fq", bad] if road == "plain_host_feed_then_device" else [bad, "s2.fq"]   # (there: bad.fq is the device route's)
    out = d / f"skip_{road}"
    p = run(d / "il", "sketch", "-t", "1", "--interleaved", *files, "-d", out, env=env)  # exit status 0
    warnings = [l for l in p.stderr.splitlines() if l.startswith("WARN") and "not mates" in l]
    assert len(warnings) == 1, p.stderr[-3000:]
    w = warnings[0]
    assert bad in w and f"records {2 * LOST} and {2 * LOST + 1} " in w and "skipping" in w, w
    assert f"'{data['lost_ids'][0]}'" in w and f"'{data['lost_ids'][1]}'" in w and data["lost_ids"][0] != data["lost_ids"][1], w
    assert not (out / f"{bad}.paired.sylsp").exists() and not (out / f"{bad}.sylsp").exists()
    assert_same_sample(read_sylsp(out / "s2.fq.paired.sylsp"), two_file(data), road)     # the other sample of the command is written


@pytest.mark.parametrize("road", ["gzip", "gzip_streamed", "fasta", "host_feed", "sequential"])
def test_no_mate_check_takes_the_records_as_they_come(data, road):
    d = data["dir"]
    name, env, _, _ = ROADS[road]
    bad = "bad" + name[1:]
    want = two_file(data, first="bad_1.fq", second="bad_2.fq", sub="lost")
    out = d / f"nocheck_{road}"
    p = run(d / "il", "sketch", "--interleaved", bad, "--no-mate-check", "-d", out, env=env)
    assert "not mates" not in p.stderr and "mates checked" not in p.stderr
    assert_same_sample(read_sylsp(out / f"{bad}.paired.sylsp"), want, road)


@pytest.fixture(scope="module")
def db(data):
    run(data["dir"], "sketch", "genome.fa", "-c", "50", "-o", data["dir"] / "db")
    return data["dir"] / "db.syldb"


def rows_without_the_sample_column(stdout):
    lines = stdout.splitlines()
    return [lines[0]] + [l.split("\t", 1)[1] for l in lines[1:]]


def two_file_rows(data, db, cmd):
    """the two-file command's TSV, made once per command"""
    key = ("rows", cmd)
    if key not in data["want"]:
        a = run(data["dir"] / "two", cmd, db, "-1", "s_1.fq", "-2", "s_2.fq", "-c", "50", exact=False)
        assert len(a.stdout.splitlines()) == 2 and "genome" in a.stdout and a.stdout.splitlines()[1].startswith("s_1.fq\t")
        data["want"][key] = a.stdout
    return data["want"][key]


STREAMED_BZIP2 = dict(SYLPH_HIP_BUNZIP2_WHOLE_MAX=str(128 << 10), SYLPH_HIP_BUNZIP2_SLICE=str(64 << 10))


@pytest.mark.parametrize("cmd", ["profile", "query"])
@pytest.mark.parametrize("name,env", [("s.fq.gz", {}), ("s.fq", {}), ("s.fa", {}), ("s.fq.bz2", STREAMED_BZIP2)])
def test_profile_and_query_print_the_two_file_rows(data, db, cmd, name, env):
    want = two_file_rows(data, db, cmd)
    b = run(data["dir"] / "il", cmd, db, "--interleaved", name, "-c", "50", env=env, exact=False)
    assert b.stdout.splitlines()[1].startswith(name + "\t"), b.stdout
    assert rows_without_the_sample_column(b.stdout) == rows_without_the_sample_column(want), (cmd, name)   # byte for byte outside the sample-file column


@pytest.mark.parametrize("cmd", ["profile", "query"])
def test_profile_and_query_skip_a_file_out_of_phase(data, db, cmd):
    """it prints no rows, the samples around it do; the order is pairs, interleaved files, single-end reads"""
    d = data["dir"]
    want = two_file_rows(data, db, cmd)
    p = run(d / "il", cmd, db, "-r", d / "two" / "s_1.fq", "--interleaved", "bad.fq.gz", "s.fq.gz", "-1", d / "two" / "s_1.fq", "-2", d / "two" / "s_2.fq", "-c", "50", exact=False)
    rows = p.stdout.splitlines()
    assert [r.split("\t")[0] for r in rows[1:]] == [str(d / "two" / "s_1.fq"), "s.fq.gz", str(d / "two" / "s_1.fq")], p.stdout
    assert rows[1].split("\t", 1)[1] == rows[2].split("\t", 1)[1] == want.splitlines()[1].split("\t", 1)[1]
    assert rows[3].split("\t", 1)[1] != rows[1].split("\t", 1)[1]                        # (mate 1 alone is another sample)
    assert p.stderr.count("not mates") == 1 and "bad.fq.gz" in p.stderr
    q = run(d / "il", cmd, db, "--interleaved", "bad.fq.gz", "--no-mate-check", "-c", "50", exact=False)
    assert len(q.stdout.splitlines()) == 2 and "not mates" not in q.stderr


def test_list_file_and_sample_names_in_job_order(data):
    d = data["dir"]
    (d / "il" / "list.txt").write_text("s.fq.gz\ns.fa\n")
    out = d / "out_names"
    run(d / "il", "sketch", "-r", d / "two" / "s_1.fq", "--lI", "list.txt", "-1", d / "two" / "s_1.fq", "-2", d / "two" / "s_2.fq",
        "-S", "the_pair", "il_gz", "il_fa", "the_single", "-d", out)
    assert sorted(os.listdir(out)) == ["il_fa.paired.sylsp", "il_gz.paired.sylsp", "the_pair.paired.sylsp", "the_single.sylsp"]
    want = two_file(data)
    for sample, file_name in (("the_pair", str(d / "two" / "s_1.fq")), ("il_gz", "s.fq.gz"), ("il_fa", "s.fa")):
        got = read_sylsp(out / f"{sample}.paired.sylsp")
        assert (got["sample_name"], got["file_name"]) == (sample, file_name)
        assert_same_sample(got, want, sample)
    single = read_sylsp(out / "the_single.sylsp")
    assert (single["sample_name"], single["file_name"], single["paired"]) == ("the_single", str(d / "two" / "s_1.fq"), False)
    p = run(d / "il", "sketch", "--lI", "list.txt", "-S", "one_name_too_few", "-d", d / "out_names2", check=False)
    assert p.returncode != 0 and "Sample name length" in p.stderr


def test_the_flags_are_options_of_all_three_commands():
    """a command line without inputs fails on the inputs, not on the options"""
    for cmd in ("sketch", "profile", "query"):
        p = subprocess.run([BIN, cmd, "--interleaved", "--no-mate-check"], capture_output=True, text=True, timeout=60)
        assert "unknown option" not in p.stderr and p.returncode != 0
