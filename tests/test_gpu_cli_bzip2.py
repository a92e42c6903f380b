"""bzip2 inputs through the command line: the reads of a sample and the genomes of a database given as .bz2 give the outputs of the
plain files — equal in everything but the recorded file names — with the device decoder (csrc/bunzip2.hip) and with the host's libbz2
reader (SYLPH_HIP_BUNZIP2_DEVICE=0); a damaged file behaves the same either way.  Fixtures are compressed here from the CLI suite's
data; no .bz2 file is committed."""
import bz2
import gzip
import struct

import pytest

from .test_gpu_cli import data, run  # noqa: F401  (the CLI suite's module fixture: E. coli slices and simulated reads)

pytestmark = pytest.mark.gpu


def _name(p):
    s = str(p).encode()
    return struct.pack("<Q", len(s)) + s


def outputs(d):
    return {f.name: f.read_bytes() for f in sorted(d.iterdir())}


def renamed(blob, names):
    """a .sylsp / .syldb with the bincode strings of the bzip2 files' names put back to the plain files' names"""
    for bz, plain in names:
        blob = blob.replace(_name(bz), _name(plain))
    return blob


@pytest.fixture(scope="module")
def bz(data):  # noqa: F811
    d = data["dir"]
    for m in ("1", "2"):
        t = (d / f"s_{m}.fq").read_bytes()
        (d / f"b_{m}.fq").write_bytes(t)
        (d / f"b_{m}.fq.bz2").write_bytes(bz2.compress(t, 9))
        (d / f"b1_{m}.fq.bz2").write_bytes(bz2.compress(t, 1))
    genomes = []
    for n in ("EC590", "K12", "O157"):
        t = gzip.decompress(open(data["genomes"][n][0], "rb").read())
        (d / f"{n}.fa").write_bytes(t)
        (d / f"{n}.fa.bz2").write_bytes(bz2.compress(t, 9))
        genomes.append((d / f"{n}.fa.bz2", d / f"{n}.fa"))
    return dict(dir=d, genomes=genomes)


def test_sketch_of_bzip2_reads_equals_plain(bz):
    d = bz["dir"]
    pairs = [(d / f"b_{m}.fq.bz2", d / f"b_{m}.fq") for m in ("1", "2")] + [(d / f"b1_{m}.fq.bz2", d / f"b_{m}.fq") for m in ("1", "2")]
    for fpr in (["--fpr", "0"], []):
        tag = "f0" if fpr else "fd"
        ref = d / f"bzp_plain_{tag}"
        run("sketch", "-1", d / "b_1.fq", "-2", d / "b_2.fq", *fpr, "-d", ref, accept_exact=False)
        want = list(outputs(ref).values())
        assert len(want) == 1
        for lv in ("", "1"):
            for dev in ("1", "0"):
                o = d / f"bzp_{tag}_{lv}_{dev}"
                p = run("sketch", "-1", d / f"b{lv}_1.fq.bz2", "-2", d / f"b{lv}_2.fq.bz2", *fpr, "-d", o, accept_exact=False,
                        env_extra={"SYLPH_HIP_BUNZIP2_DEVICE": dev, "SYLPH_HIP_FEED_TRACE": "1"})
                got = list(outputs(o).values())
                assert len(got) == 1 and renamed(got[0], pairs) == want[0], (tag, lv, dev)
                if dev == "1":
                    assert "bzip2 decoded on the device" in p.stderr, p.stderr[-2000:]
                    dev_bytes = got[0]
                else:
                    assert got[0] == dev_bytes
    # single-end
    ref = d / "bzr_plain"
    run("sketch", "-r", d / "b_1.fq", "-d", ref)
    for dev in ("1", "0"):
        o = d / f"bzr_{dev}"
        run("sketch", "-r", d / "b_1.fq.bz2", "-d", o, env_extra={"SYLPH_HIP_BUNZIP2_DEVICE": dev})
        assert [renamed(x, pairs) for x in outputs(o).values()] == list(outputs(ref).values())


def test_database_from_bzip2_genomes_equals_plain(bz):
    d = bz["dir"]
    gs = bz["genomes"]
    run("sketch", "-g", *[p for _, p in gs], "-o", d / "bzdb_plain")
    run("sketch", "-g", *[b for b, _ in gs], "-o", d / "bzdb_bz")
    a = (d / "bzdb_plain.syldb").read_bytes()
    b = (d / "bzdb_bz.syldb").read_bytes()
    assert renamed(b, gs) == a and len(a) > 1000


def test_profile_and_query_on_bzip2_reads(bz):
    d = bz["dir"]
    gs = bz["genomes"]
    run("sketch", "-g", *[p for _, p in gs], "-o", d / "bzq_db")
    db = d / "bzq_db.syldb"
    for cmd in ("profile", "query"):
        a = run(cmd, db, "-1", d / "b_1.fq", "-2", d / "b_2.fq", "-r", d / "b_1.fq").stdout
        for dev in ("1", "0"):
            b = run(cmd, db, "-1", d / "b_1.fq.bz2", "-2", d / "b_2.fq.bz2", "-r", d / "b_1.fq.bz2",
                    env_extra={"SYLPH_HIP_BUNZIP2_DEVICE": dev}).stdout
            b = b.replace(str(d / "b_1.fq.bz2"), str(d / "b_1.fq")).replace(str(d / "b_2.fq.bz2"), str(d / "b_2.fq"))
            assert sorted(a.strip().split("\n")) == sorted(b.strip().split("\n")), (cmd, dev)
            assert len(a.strip().split("\n")) >= 2


def test_damaged_bzip2_goes_the_host_way(bz):
    d = bz["dir"]
    good = (d / "b_1.fq.bz2").read_bytes()
    (d / "trunc.fq.bz2").write_bytes(good[: len(good) * 2 // 3])
    (d / "flipped.fq.bz2").write_bytes(good[:5000] + bytes([good[5000] ^ 0x40]) + good[5001:])
    (d / "single.fq.bz2").write_bytes(bz2.compress((d / "b_2.fq").read_bytes(), 5))
    res = {}
    for dev in ("1", "0"):
        o = d / f"bz_damaged_{dev}"
        p = run("sketch", "-t", "1", "-r", d / "b_1.fq", d / "trunc.fq.bz2", d / "flipped.fq.bz2", d / "single.fq.bz2", "-d", o, check=False,
                env_extra={"SYLPH_HIP_BUNZIP2_DEVICE": dev, "SYLPH_HIP_FEED_TRACE": "1"})
        res[dev] = (p.returncode, outputs(o), sorted(ln for ln in p.stderr.split("\n") if "WARN" in ln or "ERROR" in ln))
        if dev == "1":
            assert p.stderr.count("device bunzip2 declined") == 2 and p.stderr.count("bzip2 decoded on the device") == 1, p.stderr[-3000:]
    assert res["1"] == res["0"] and "single.fq.bz2.sylsp" in res["1"][1]


def test_sketch_of_bzip2_over_several_gpus_equals_one_gpu(bz):
    d = bz["dir"]
    firsts = [d / "b_1.fq.bz2", d / "b1_1.fq.bz2", d / "b_1.fq.bz2"]
    seconds = [d / "b_2.fq.bz2", d / "b1_2.fq.bz2", d / "b_2.fq.bz2"]
    one, many = d / "bzg_one", d / "bzg_many"
    run("sketch", "-1", *firsts[:2], "-2", *seconds[:2], "-r", d / "b_1.fq.bz2", "-t", "1", "-d", one)
    p = run("sketch", "-1", *firsts[:2], "-2", *seconds[:2], "-r", d / "b_1.fq.bz2", "-t", "2", "--gpus", "2", "-d", many,
            env_extra={"SYLPH_HIP_FAKE_GPUS": "2"})
    assert "sketch worker 1 runs on GPU 1" in p.stderr, p.stderr[-2000:]
    a, b = outputs(one), outputs(many)
    assert a == b and len(a) == 3
