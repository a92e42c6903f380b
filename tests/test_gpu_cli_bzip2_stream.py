"""`sylph-hip` on bzip2 samples that go the STREAM route (host/sample_feed.cpp sketch_streamed over sylph_bunzip2_stream_*): with
SYLPH_HIP_BUNZIP2_WHOLE_MAX lowered a pair of 3 MB mates is "too large for the whole-file road" and is decoded on the device one
128 KiB slice per mate at a time; SYLPH_HIP_BUNZIP2_STREAM=1 streams whatever the size, =0 never.  Pairs and single-end samples, FASTQ
and FASTA: what is written must be byte-identical to what the plain files and the whole-file road give; the feed trace says which
road a sample took and in how many slices."""
import bz2
import os
import re
import subprocess

import numpy as np
import pytest

from .helpers import random_seq, revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sylph_amd", "sylph-hip")
STREAM_ENV = dict(SYLPH_HIP_BUNZIP2_WHOLE_MAX=str(256 << 10), SYLPH_HIP_BUNZIP2_SLICE=str(128 << 10))
STREAM_LINE = re.compile(r"stream route: bzip2 decoded on the device in (\d+) slices \((\d+) (FASTA|FASTQ) records")
WHOLE_LINE = "device route: bzip2 decoded on the device"
KINDS = ("fq", "fa")


def reads_text(rng, genome, n, mate, fasta):
    """n reads of 100-150 bases of the genome as four-line FASTQ (qualities of a few values in runs) or as FASTA records"""
    out = []
    qa = np.frombuffer(b"FFFFFFFF:,#", dtype=np.uint8)
    for i in range(n):
        L = int(rng.integers(100, 151))
        s = int(rng.integers(0, len(genome) - L))
        seq = genome[s:s + L] if rng.random() < 0.5 else revcomp(genome[s:s + L])
        name = b"A00123:45:HXXXXXXXX:1:%d:%d:%d %d:N:0:ACGT\n" % (1101 + i // 9000, 1000 + (i * 37) % 30000, i, mate)
        if fasta:
            out.append(b">" + name + bytes(seq) + b"\n")
        else:
            q = np.repeat(rng.choice(qa, size=L // 7 + 1), 7)[:L]
            out.append(b"@" + name + bytes(seq) + b"\n+\n" + q.tobytes() + b"\n")
    return b"".join(out)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """Directories with files of the same names (a sketch records its file's name): plain/ holds the text, bz/ the same text through
    bzip2 -9 (mate 1 as two streams, as pbzip2 would write it), bad/ a shorter pair whose mate 2 has a flipped bit in a late block.
    Mate 2 has fewer records than mate 1."""
    d = tmp_path_factory.mktemp("cli_bzip2_stream")
    rng = np.random.default_rng(78)
    genome = random_seq(rng, 150000)
    for sub in ("plain", "bz", "bad"):
        (d / sub).mkdir()
    for kind in KINDS:
        n1, n2 = (11000, 10300) if kind == "fq" else (9000, 8600)
        m1, m2 = reads_text(rng, genome, n1, 1, kind == "fa"), reads_text(rng, genome, n2, 2, kind == "fa")
        (d / "plain" / f"s_1.{kind}").write_bytes(m1)
        (d / "plain" / f"s_2.{kind}").write_bytes(m2)
        half = m1.index(b"\n@" if kind == "fq" else b"\n>", len(m1) // 2) + 1
        b1, b2 = bz2.compress(m1[:half], 9) + bz2.compress(m1[half:], 9), bz2.compress(m2, 9)
        assert len(b1) > (256 << 10) and len(b2) > (256 << 10)
        (d / "bz" / f"s_1.{kind}").write_bytes(b1)
        (d / "bz" / f"s_2.{kind}").write_bytes(b2)
    m1, m2 = (d / "plain" / "s_1.fq").read_bytes(), (d / "plain" / "s_2.fq").read_bytes()
    bad = bytearray(bz2.compress(m2, 1))
    assert len(bad) > 5 * (64 << 10)
    bad[len(bad) - (40 << 10)] ^= 0x10                                                # mate 2: a flipped bit in a late block, seen in a late slice
    (d / "bad" / "s_1.fq").write_bytes(bz2.compress(m1, 1))
    (d / "bad" / "s_2.fq").write_bytes(bytes(bad))
    with open(d / "genome.fa", "wb") as f:
        f.write(b">genome\n" + bytes(genome) + b"\n")
    return d


def run(cwd, *args, env=None, check=True):
    e = dict(os.environ, SYLPH_HIP_FEED_TRACE="1", SYLPH_HIP_EXACT_DEDUP="1")
    for k in ("SYLPH_HIP_BUNZIP2_STREAM", "SYLPH_HIP_BUNZIP2_WHOLE_MAX", "SYLPH_HIP_BUNZIP2_SLICE"):
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=e, cwd=str(cwd))
    if check:
        assert p.returncode == 0, p.stderr[-3000:]
    return p


@pytest.fixture(scope="module")
def db(data):
    run(data, "sketch", "genome.fa", "-c", "50", "-o", data / "db")
    return data / "db.syldb"


def slices_of(p, kind=None):
    m = STREAM_LINE.search(p.stderr)
    if m and kind:
        assert m.group(3) == ("FASTA" if kind == "fa" else "FASTQ")
    return int(m.group(1)) if m else 0


@pytest.mark.parametrize("kind", KINDS)
def test_a_streamed_pair_gives_the_sketch_of_the_plain_files_and_of_the_whole_file_road(data, kind):
    d = data
    pair = ("-1", f"s_1.{kind}", "-2", f"s_2.{kind}", "--fpr", "0")
    out = f"s_1.{kind}.paired.sylsp"
    run(d / "plain", "sketch", *pair, "-d", d / f"out_plain_{kind}")
    want = (d / f"out_plain_{kind}" / out).read_bytes()
    assert len(want) > 1000
    whole = run(d / "bz", "sketch", *pair, "-d", d / f"out_whole_{kind}")
    assert WHOLE_LINE in whole.stderr and not slices_of(whole)                       # by default every sample the whole-file road takes still takes it
    assert (d / f"out_whole_{kind}" / out).read_bytes() == want
    st = run(d / "bz", "sketch", *pair, "-d", d / f"out_stream_{kind}", env=STREAM_ENV)
    assert slices_of(st, kind) > 2 and WHOLE_LINE not in st.stderr, st.stderr[-2000:]  # the trace names the stream route and its slices
    assert (d / f"out_stream_{kind}" / out).read_bytes() == want
    # asked for, the stream also takes what the whole-file road would have
    st = run(d / "bz", "sketch", *pair, "-d", d / f"out_stream1_{kind}", env=dict(SYLPH_HIP_BUNZIP2_STREAM="1", SYLPH_HIP_BUNZIP2_SLICE=str(256 << 10)))
    assert slices_of(st, kind) > 1 and (d / f"out_stream1_{kind}" / out).read_bytes() == want


@pytest.mark.parametrize("kind", KINDS)
def test_a_streamed_single_end_sample(data, kind):
    d = data
    run(d / "plain", "sketch", "-r", f"s_1.{kind}", "-d", d / f"single_plain_{kind}")
    want = (d / f"single_plain_{kind}" / f"s_1.{kind}.sylsp").read_bytes()
    whole = run(d / "bz", "sketch", "-r", f"s_1.{kind}", "-d", d / f"single_whole_{kind}")
    assert WHOLE_LINE in whole.stderr and (d / f"single_whole_{kind}" / f"s_1.{kind}.sylsp").read_bytes() == want
    st = run(d / "bz", "sketch", "-r", f"s_1.{kind}", "-d", d / f"single_stream_{kind}", env=STREAM_ENV)
    assert slices_of(st, kind) > 1, st.stderr[-2000:]
    assert len(want) > 1000 and (d / f"single_stream_{kind}" / f"s_1.{kind}.sylsp").read_bytes() == want


@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_profile_of_a_streamed_sample(data, db, kind, paired):
    d = data
    sample = ("-1", f"s_1.{kind}", "-2", f"s_2.{kind}") if paired else ("-r", f"s_2.{kind}")
    a = run(d / "plain", "profile", db, *sample, "-c", "50")
    b = run(d / "bz", "profile", db, *sample, "-c", "50", env=STREAM_ENV)
    assert slices_of(b, kind) > 1, b.stderr[-2000:]
    assert len(a.stdout.splitlines()) == 2 and "genome" in a.stdout                 # the header and the genome's row
    assert a.stdout == b.stdout                                                     # (the files' names are the same in both directories)


def test_with_the_stream_off_the_sample_goes_the_host_road(data):
    d = data
    pair = ("-1", "s_1.fq", "-2", "s_2.fq", "--fpr", "0")
    run(d / "plain", "sketch", *pair, "-d", d / "off_plain")
    p = run(d / "bz", "sketch", *pair, "-d", d / "off", env=dict(STREAM_ENV, SYLPH_HIP_BUNZIP2_STREAM="0"))
    assert not slices_of(p) and WHOLE_LINE not in p.stderr and "the stream is off" in p.stderr, p.stderr[-2000:]
    assert (d / "off" / "s_1.fq.paired.sylsp").read_bytes() == (d / "off_plain" / "s_1.fq.paired.sylsp").read_bytes()


def test_a_pair_damaged_in_a_late_slice_gives_what_the_host_road_gives(data):
    d = data
    pair = ("-1", "s_1.fq", "-2", "s_2.fq", "--fpr", "0")
    host = run(d / "bad", "sketch", *pair, "-d", d / "bad_host", env=dict(SYLPH_HIP_BUNZIP2_DEVICE="0"), check=False)
    st = run(d / "bad", "sketch", *pair, "-d", d / "bad_stream", env=dict(SYLPH_HIP_BUNZIP2_STREAM="1", SYLPH_HIP_BUNZIP2_SLICE=str(64 << 10)), check=False)
    assert "stream route declined" in st.stderr and "sylph_bunzip2_stream_next" in st.stderr and not slices_of(st), st.stderr[-2000:]
    assert st.returncode == host.returncode
    a, b = d / "bad_host" / "s_1.fq.paired.sylsp", d / "bad_stream" / "s_1.fq.paired.sylsp"
    assert a.exists() == b.exists()
    if a.exists():
        assert a.read_bytes() == b.read_bytes()
