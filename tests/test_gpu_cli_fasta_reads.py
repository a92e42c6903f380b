"""`sylph-hip sketch|profile -r/-1/-2` on FASTA-format READ files (host/sample_feed.cpp over sylph_fasta_index[_window] and
sylph_sketch_push_fasta): the same reads as plain FASTA, gzip, bzip2 and plain FASTQ under the same file names.  What the device routes
write must be byte-identical to what the host reader writes (SYLPH_HIP_FASTA_READS_DEVICE=0) and to the FASTQ files' sketches; the feed
trace must name the FASTA device route; a pair of mixed kinds and a FASTA with a stray '\\r' stay with the host road, with its output
and its messages."""
import bz2
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from .helpers import random_seq, revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sylph_amd", "sylph-hip")
STREAM_ENV = dict(SYLPH_HIP_INFLATE_WHOLE_MAX=str(1 << 20), SYLPH_HIP_INFLATE_SLICE=str(128 << 10))
STREAM_LINE = re.compile(r"stream route: gzip inflated on the device in (\d+) slices \((\d+) FASTA records")
FASTA_LINE = "device route: FASTA records found"
KINDS = ("fa", "gz", "bz2")
DECODED_LINE = {"gz": "device route: gzip inflated on the device", "bz2": "device route: bzip2 decoded on the device"}


def the_reads(rng, genome, n_short, n_long):
    reads = []
    for i in range(n_short + n_long):
        L = int(rng.integers(100, 151)) if i < n_short else int(rng.integers(2000, 12001))
        s = int(rng.integers(0, len(genome) - L))
        reads.append(bytes(genome[s:s + L] if rng.random() < 0.5 else revcomp(genome[s:s + L])))
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    for i in range(7, len(reads), 23):                                              # exact copies: the dedup has work
        reads[i] = reads[i - 1]
    return reads


def as_fasta(reads, mate):
    return b"".join(b">read%d/%d\n" % (i, mate) + b"".join(r[j:j + 70] + b"\n" for j in range(0, len(r), 70)) for i, r in enumerate(reads))


def as_fastq(reads, mate):
    return b"".join(b"@read%d/%d\n" % (i, mate) + r + b"\n+\n" + b"F" * len(r) + b"\n" for i, r in enumerate(reads))


def gz6(data):
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    return co.compress(data) + co.flush()


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """One directory per kind with files of the same names (a sketch records its file's name): fa/ plain FASTA (70 bases per line), gz/
    the same through gzip -6, bz2/ through bzip2, fq/ the same reads as plain FASTQ; mixed/ a gzip FASTA mate 1 beside a gzip FASTQ mate 2;
    cr/ a FASTA with a '\\r' inside a sequence line.  Mate 2 holds fewer records than mate 1."""
    d = tmp_path_factory.mktemp("cli_fasta_reads")
    rng = np.random.default_rng(91)
    genome = random_seq(rng, 150000)
    r1, r2 = the_reads(rng, genome, 20000, 60), the_reads(rng, genome, 19400, 55)
    t1, t2 = as_fasta(r1, 1), as_fasta(r2, 2)
    assert 2_700_000 < len(t2) < len(t1) < 3_600_000
    pack = {"fa": lambda t: t, "gz": gz6, "bz2": bz2.compress}
    for kind in KINDS:
        (d / kind).mkdir()
        (d / kind / "s_1.fx").write_bytes(pack[kind](t1))
        (d / kind / "s_2.fx").write_bytes(pack[kind](t2))
    (d / "fq").mkdir()
    (d / "fq" / "s_1.fx").write_bytes(as_fastq(r1, 1))
    (d / "fq" / "s_2.fx").write_bytes(as_fastq(r2, 2))
    (d / "mixed").mkdir()
    (d / "mixed" / "s_1.fx").write_bytes(gz6(t1))
    (d / "mixed" / "s_2.fx").write_bytes(gz6(as_fastq(r2, 2)))
    (d / "cr").mkdir()
    at = t1.index(b"\n", 100000) - 20
    (d / "cr" / "s_1.fx").write_bytes(t1[:at] + b"\r" + t1[at:])
    (d / "cr" / "s_2.fx").write_bytes(t1)
    with open(d / "genome.fa", "wb") as f:
        f.write(b">genome\n" + bytes(genome) + b"\n")
    return d


def run(cwd, *args, device="1", env=None, check=True):
    e = dict(os.environ, SYLPH_HIP_FEED_TRACE="1", SYLPH_HIP_EXACT_DEDUP="1", SYLPH_HIP_FASTA_READS_DEVICE=device)
    for name in ("SYLPH_HIP_INFLATE_STREAM", "SYLPH_HIP_FEED_DEVICE", "SYLPH_HIP_INFLATE_DEVICE", "SYLPH_HIP_BUNZIP2_DEVICE"):
        e.pop(name, None)
    e.update(env or {})
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=e, cwd=str(cwd))
    if check:
        assert p.returncode == 0, p.stderr[-3000:]
    return p


def messages(p):
    """the command's own messages: everything but the trace's lines and the timing notes, the output directory's name taken out"""
    out = p.args[p.args.index("-d") + 1] if "-d" in p.args else ""
    return [ln.replace(out, "OUT") if out else ln for ln in p.stderr.splitlines() if not ln.startswith("[sylph_hip") and "timing:" not in ln]


def took_the_fasta_route(p, kind):
    return FASTA_LINE in p.stderr and (kind == "fa" or DECODED_LINE[kind] in p.stderr)


@pytest.mark.parametrize("kind", KINDS)
def test_single_end_samples(data, kind):
    """two samples in one command, one after the other (-t 1): the first finds the engine coming up, the second finds it up"""
    d = data
    files = ("-r", "s_2.fx", "s_1.fx", "-t", "1")
    fq = run(d / "fq", "sketch", *files, "-d", d / "r_fq")
    dev = run(d / kind, "sketch", *files, "-d", d / f"r_dev_{kind}")
    host = run(d / kind, "sketch", *files, "-d", d / f"r_host_{kind}", device="0")
    assert took_the_fasta_route(dev, kind), dev.stderr[-3000:]
    assert FASTA_LINE not in host.stderr and "FASTA reads stay on the host reader" in host.stderr, host.stderr[-3000:]
    for name in ("s_1.fx.sylsp", "s_2.fx.sylsp"):
        want = (d / f"r_host_{kind}" / name).read_bytes()
        assert len(want) > 1000
        assert (d / f"r_dev_{kind}" / name).read_bytes() == want, name
        assert (d / "r_fq" / name).read_bytes() == want, name
    assert messages(dev) == messages(host)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fpr", [("--fpr", "0"), ()])
def test_pairs(data, kind, fpr):
    d = data
    tag = f"{kind}_{len(fpr)}"
    pairs = ("-1", "s_1.fx", "-2", "s_2.fx")            # (one sample: a plain FASTA pair waits for the engine as a compressed one does)
    fq = run(d / "fq", "sketch", *pairs, *fpr, "-d", d / f"p_fq_{tag}")
    dev = run(d / kind, "sketch", *pairs, *fpr, "-d", d / f"p_dev_{tag}")
    host = run(d / kind, "sketch", *pairs, *fpr, "-d", d / f"p_host_{tag}", device="0")
    assert took_the_fasta_route(dev, kind), dev.stderr[-3000:]
    assert FASTA_LINE not in host.stderr and FASTA_LINE not in fq.stderr
    want = (d / f"p_host_{tag}" / "s_1.fx.paired.sylsp").read_bytes()
    assert len(want) > 1000
    assert (d / f"p_dev_{tag}" / "s_1.fx.paired.sylsp").read_bytes() == want
    assert (d / f"p_fq_{tag}" / "s_1.fx.paired.sylsp").read_bytes() == want
    assert messages(dev) == messages(host)


def test_a_gzip_pair_through_the_stream(data):
    d = data
    pair = ("-1", "s_1.fx", "-2", "s_2.fx", "--fpr", "0")
    host = run(d / "gz", "sketch", *pair, "-d", d / "st_host", device="0")
    st = run(d / "gz", "sketch", *pair, "-d", d / "st_dev", env=STREAM_ENV)
    m = STREAM_LINE.search(st.stderr)
    assert m and int(m.group(1)) > 1 and int(m.group(2)) == 19455 and DECODED_LINE["gz"] not in st.stderr, st.stderr[-3000:]
    assert (d / "st_dev" / "s_1.fx.paired.sylsp").read_bytes() == (d / "st_host" / "s_1.fx.paired.sylsp").read_bytes()
    off = run(d / "gz", "sketch", *pair, "-d", d / "st_off", device="0", env=STREAM_ENV)      # ... and with FASTA reads kept on the host
    assert not STREAM_LINE.search(off.stderr) and "FASTA reads stay on the host reader" in off.stderr
    assert (d / "st_off" / "s_1.fx.paired.sylsp").read_bytes() == (d / "st_host" / "s_1.fx.paired.sylsp").read_bytes()


@pytest.mark.parametrize("kind", KINDS)
def test_profile_of_a_pair(data, kind):
    d = data
    if not (d / "db.syldb").exists():
        run(d, "sketch", "genome.fa", "-c", "50", "-o", d / "db")
    pair = ("-1", "s_1.fx", "-2", "s_2.fx", "-c", "50")
    dev = run(d / kind, "profile", d / "db.syldb", *pair)
    host = run(d / kind, "profile", d / "db.syldb", *pair, device="0")
    assert took_the_fasta_route(dev, kind), dev.stderr[-3000:]
    assert len(host.stdout.splitlines()) >= 2 and "genome" in host.stdout
    assert dev.stdout == host.stdout


def test_a_pair_of_a_fasta_and_a_fastq_mate_stays_with_the_host_road(data):
    d = data
    pair = ("-1", "s_1.fx", "-2", "s_2.fx", "--fpr", "0")
    dev = run(d / "mixed", "sketch", *pair, "-d", d / "mixed_dev")
    off = run(d / "mixed", "sketch", *pair, "-d", d / "mixed_off", env=dict(SYLPH_HIP_FEED_DEVICE="0"))
    assert "one mate is FASTA, the other is not" in dev.stderr and FASTA_LINE not in dev.stderr, dev.stderr[-3000:]
    want = (d / "mixed_off" / "s_1.fx.paired.sylsp").read_bytes()
    assert len(want) > 1000 and (d / "mixed_dev" / "s_1.fx.paired.sylsp").read_bytes() == want
    assert messages(dev) == messages(off)


def test_a_fasta_with_a_stray_cr_gives_the_host_roads_output_and_messages(data):
    d = data
    files = ("-r", "s_2.fx", "s_1.fx", "-t", "1")
    dev = run(d / "cr", "sketch", *files, "-d", d / "cr_dev", check=False)
    host = run(d / "cr", "sketch", *files, "-d", d / "cr_host", device="0", check=False)
    assert "device route declined" in dev.stderr and "'\\r'" in dev.stderr, dev.stderr[-3000:]
    assert dev.returncode == host.returncode and messages(dev) == messages(host)
    for name in ("s_1.fx.sylsp", "s_2.fx.sylsp"):
        a, b = d / "cr_dev" / name, d / "cr_host" / name
        assert a.exists() == b.exists()
        if a.exists():
            assert a.read_bytes() == b.read_bytes()


def test_fasta_reads_from_a_named_pipe_go_through_the_host_reader(data):
    """A sample that is not a regular file can be read once, front to back: the route may not peek at its first byte."""
    import threading
    d = data
    (d / "pipe").mkdir()
    fifo = d / "pipe" / "p_1.fx"
    os.mkfifo(fifo)
    text = (d / "fa" / "s_1.fx").read_bytes()

    def feed():
        with open(fifo, "wb") as f:
            f.write(text)
    t = threading.Thread(target=feed, daemon=True)
    t.start()
    e = dict(os.environ, SYLPH_HIP_FEED_TRACE="1", SYLPH_HIP_FASTA_READS_DEVICE="1")
    p = subprocess.run([BIN, "sketch", "-r", str(fifo), "-d", str(d / "pipe_out")], capture_output=True, text=True, timeout=120, env=e, cwd=str(d))
    t.join(timeout=60)
    assert p.returncode == 0 and FASTA_LINE not in p.stderr, p.stderr[-2000:]
    run(d / "fa", "sketch", "-r", "s_1.fx", "-d", d / "pipe_out")
    a, b = (d / "pipe_out" / "p_1.fx.sylsp").read_bytes(), (d / "pipe_out" / "s_1.fx.sylsp").read_bytes()
    n_tab = 8 + 12 * int.from_bytes(b[:8], "little")
    assert n_tab > 1000 and a[:n_tab] == b[:n_tab]
