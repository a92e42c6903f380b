"""`sylph-hip` on gzip samples that go the STREAM route (host/sample_feed.cpp sketch_gzip_streamed over sylph_inflate_stream_*): with
SYLPH_HIP_INFLATE_WHOLE_MAX lowered to 1 MiB a pair of 3 MB mates is "too large for the whole-file road" and is inflated on the device
one 128 KiB slice per mate at a time.  What is written must be byte-identical to what the plain files and the whole-file road give;
the feed trace says which road a sample took and in how many slices."""
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
STREAM_LINE = re.compile(r"stream route: gzip inflated on the device in (\d+) slices")
WHOLE_LINE = "device route: gzip inflated on the device"


def reads_text(rng, genome, n, mate):
    """four-line FASTQ of n reads of 100-150 bases of the genome, qualities of a few values in runs (deflate blocks of ~30 KB)"""
    out = []
    qa = np.frombuffer(b"FFFFFFFF:,#", dtype=np.uint8)
    for i in range(n):
        L = int(rng.integers(100, 151))
        s = int(rng.integers(0, len(genome) - L))
        seq = genome[s:s + L] if rng.random() < 0.5 else revcomp(genome[s:s + L])
        q = np.repeat(rng.choice(qa, size=L // 7 + 1), 7)[:L]
        out.append(b"@A00123:45:HXXXXXXXX:1:%d:%d:%d %d:N:0:ACGT\n" % (1101 + i // 9000, 1000 + (i * 37) % 30000, i, mate) + bytes(seq) + b"\n+\n" + q.tobytes() + b"\n")
    return b"".join(out)


def gz6(data):
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    return co.compress(data) + co.flush()


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """Two directories with files of the same names (a sketch records its file's name): plain/ holds the text, gz/ the same text through
    gzip -6.  Mate 2 has fewer records than mate 1."""
    d = tmp_path_factory.mktemp("cli_stream")
    rng = np.random.default_rng(77)
    genome = random_seq(rng, 150000)
    m1, m2 = reads_text(rng, genome, 11000, 1), reads_text(rng, genome, 10300, 2)       # ~3 MB each
    assert len(m1) > 2_800_000 and len(m2) > 2_600_000
    for sub in ("plain", "gz", "bad"):
        (d / sub).mkdir()
    (d / "plain" / "s_1.fq").write_bytes(m1)
    (d / "plain" / "s_2.fq").write_bytes(m2)
    g1, g2 = gz6(m1), gz6(m2)
    assert len(g1) + len(g2) > (1 << 20)
    (d / "gz" / "s_1.fq").write_bytes(g1)
    (d / "gz" / "s_2.fq").write_bytes(g2)
    # (the damaged pair is a third of the sample: what the host reader does with a damaged gzip file takes it seconds per MB)
    b1, b2 = gz6(m1[:len(m1) // 3]), gz6(m2[:len(m2) // 3])
    bad = bytearray(b2)
    bad[-8] ^= 1                                                                      # mate 2: a wrong CRC, seen in its last slice
    (d / "bad" / "s_1.fq").write_bytes(b1)
    (d / "bad" / "s_2.fq").write_bytes(bytes(bad))
    with open(d / "genome.fa", "wb") as f:
        f.write(b">genome\n" + bytes(genome) + b"\n")
    return d


def run(cwd, *args, env=None, check=True):
    e = dict(os.environ, SYLPH_HIP_FEED_TRACE="1", SYLPH_HIP_EXACT_DEDUP="1")
    e.pop("SYLPH_HIP_INFLATE_STREAM", None)
    e.update(env or {})
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=e, cwd=str(cwd))
    if check:
        assert p.returncode == 0, p.stderr[-3000:]
    return p


def slices_of(p):
    m = STREAM_LINE.search(p.stderr)
    return int(m.group(1)) if m else 0


def test_a_streamed_pair_gives_the_sketch_of_the_plain_files_and_of_the_whole_file_road(data):
    d = data
    pair = ("-1", "s_1.fq", "-2", "s_2.fq", "--fpr", "0")
    run(d / "plain", "sketch", *pair, "-d", d / "out_plain")
    want = (d / "out_plain" / "s_1.fq.paired.sylsp").read_bytes()
    assert len(want) > 1000
    whole = run(d / "gz", "sketch", *pair, "-d", d / "out_whole")
    assert WHOLE_LINE in whole.stderr and not slices_of(whole)
    assert (d / "out_whole" / "s_1.fq.paired.sylsp").read_bytes() == want
    st = run(d / "gz", "sketch", *pair, "-d", d / "out_stream", env=STREAM_ENV)
    assert slices_of(st) > 1 and WHOLE_LINE not in st.stderr, st.stderr[-2000:]      # the trace names the stream route, with more than one slice
    assert (d / "out_stream" / "s_1.fq.paired.sylsp").read_bytes() == want
    # asked for, the stream also takes what the whole-file road would have
    st = run(d / "gz", "sketch", *pair, "-d", d / "out_stream1", env=dict(SYLPH_HIP_INFLATE_STREAM="1", SYLPH_HIP_INFLATE_SLICE=str(256 << 10)))
    assert slices_of(st) > 1 and (d / "out_stream1" / "s_1.fq.paired.sylsp").read_bytes() == want


def test_a_streamed_single_end_sample(data):
    d = data
    run(d / "plain", "sketch", "-r", "s_1.fq", "-d", d / "single_plain")
    want = (d / "single_plain" / "s_1.fq.sylsp").read_bytes()
    st = run(d / "gz", "sketch", "-r", "s_1.fq", "-d", d / "single_stream", env=dict(STREAM_ENV, SYLPH_HIP_INFLATE_WHOLE_MAX=str(1 << 19)))
    assert slices_of(st) > 1, st.stderr[-2000:]
    assert len(want) > 1000 and (d / "single_stream" / "s_1.fq.sylsp").read_bytes() == want


def test_profile_of_a_streamed_pair(data):
    d = data
    run(d, "sketch", "genome.fa", "-c", "50", "-o", d / "db")
    pair = ("-1", "s_1.fq", "-2", "s_2.fq", "-c", "50")
    a = run(d / "plain", "profile", d / "db.syldb", *pair)
    b = run(d / "gz", "profile", d / "db.syldb", *pair, env=STREAM_ENV)
    assert slices_of(b) > 1, b.stderr[-2000:]
    assert len(a.stdout.splitlines()) == 2 and "genome" in a.stdout                     # the header and the genome's row
    assert a.stdout == b.stdout


def test_with_the_stream_off_the_sample_goes_the_host_road(data):
    d = data
    pair = ("-1", "s_1.fq", "-2", "s_2.fq", "--fpr", "0")
    run(d / "plain", "sketch", *pair, "-d", d / "off_plain")
    p = run(d / "gz", "sketch", *pair, "-d", d / "off", env=dict(STREAM_ENV, SYLPH_HIP_INFLATE_STREAM="0"))
    assert not slices_of(p) and WHOLE_LINE not in p.stderr and "the stream is off" in p.stderr, p.stderr[-2000:]
    assert (d / "off" / "s_1.fq.paired.sylsp").read_bytes() == (d / "off_plain" / "s_1.fq.paired.sylsp").read_bytes()


def test_a_pair_damaged_in_a_late_slice_gives_what_the_host_road_gives(data):
    d = data
    pair = ("-1", "s_1.fq", "-2", "s_2.fq", "--fpr", "0")
    host = run(d / "bad", "sketch", *pair, "-d", d / "bad_host", env=dict(SYLPH_HIP_INFLATE_DEVICE="0"), check=False)
    st = run(d / "bad", "sketch", *pair, "-d", d / "bad_stream", env=dict(SYLPH_HIP_INFLATE_WHOLE_MAX=str(256 << 10), SYLPH_HIP_INFLATE_SLICE=str(64 << 10)), check=False)
    assert "stream route declined" in st.stderr and not slices_of(st), st.stderr[-2000:]
    assert st.returncode == host.returncode
    a, b = d / "bad_host" / "s_1.fq.paired.sylsp", d / "bad_stream" / "s_1.fq.paired.sylsp"
    assert a.exists() == b.exists()
    if a.exists():
        assert a.read_bytes() == b.read_bytes()
