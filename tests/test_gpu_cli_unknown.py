"""GPU tests of `sylph-hip profile -u` / `query -u` with the walks over the sample's counts counted on the device
(SYLPH_HIP_UNKNOWN_DEVICE=1 / only: the pipeline's option "table_summary", csrc/table_summary.hip) against the host's walk over the
copied table (=0) and the default: the same bytes on stdout, the same --estimate-unknown messages.  Inputs are
tests/test_gpu_cli_bootstrap.py's: reads at full and at thinned coverage (the thinned ones take the fixed 99.5 % identity), as
raw pairs, as a single-end sample and as sketch files."""
import os
import re
import subprocess

import pytest

from .test_gpu_cli_bootstrap import build_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sylph_amd", "sylph-hip")
MESSAGE = re.compile(r"estimate-unknown|short-read sample has high diversity|% of reads detected in database|within 10% of the limit|genomes passing profiling")
TRACE = re.compile(r"^\[sylph_hip feed\] unknown (\S+): road ([a-z ()]+), rung (\d+), (\d+) chunks walked again$", re.M)


def run(*args, unknown=None, **env):
    e = dict(os.environ, SYLPH_HIP_EXACT_DEDUP="1", **env)
    for k in ("SYLPH_HIP_UNKNOWN_DEVICE", "SYLPH_HIP_TABLE_SUMMARY_CAPS", "SYLPH_HIP_TABLE_SUMMARY_CHUNK"):
        if k not in env:
            e.pop(k, None)
    if unknown is not None:
        e["SYLPH_HIP_UNKNOWN_DEVICE"] = unknown
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=e)


def messages(p):
    """the lines -u adds to or changes on stderr"""
    return [l for l in p.stderr.split("\n") if MESSAGE.search(l)]


@pytest.fixture(scope="module")
def data(tmp_path_factory, golden_dir):
    d = build_inputs(tmp_path_factory.mktemp("cli_unknown"), golden_dir)
    out = d["dir"]
    for reads in ("s", "thin"):
        p = run("sketch", "-c", "50", "-d", out, "-1", out / f"{reads}_1.fq", "-2", out / f"{reads}_2.fq")
        assert p.returncode == 0, p.stderr[-3000:]
    d["sylsp"] = [out / "s_1.fq.paired.sylsp", out / "thin_1.fq.paired.sylsp"]
    assert all(os.path.exists(p) for p in d["sylsp"])
    return d


def samples(data, kind):
    d = data["dir"]
    if kind == "sylsp":
        return tuple(data["sylsp"])
    if kind == "single":
        return ("-r", d / "s_1.fq")
    return ("-1", d / "s_1.fq", d / "thin_1.fq", "-2", d / "s_2.fq", d / "thin_2.fq")


@pytest.mark.parametrize("seq_id", [(), ("-I", "99.1")], ids=["walk", "I"])
@pytest.mark.parametrize("kind", ["raw", "single", "sylsp"])
@pytest.mark.parametrize("command", ["profile", "query"])
def test_device_road_prints_the_hosts_bytes_and_messages(data, command, kind, seq_id):
    """stdout and the -u messages for SYLPH_HIP_UNKNOWN_DEVICE = 0 and only — and, for the sketch files, unset — byte for byte (=1: the
    next test)"""
    args = (command, data["db"], "-c", "50", "-u") + samples(data, kind) + seq_id
    runs = [run(*args, unknown=u, SYLPH_HIP_DEBUG="1") for u in ("0", "only") + ((None,) if kind == "sylsp" else ())]
    for p in runs:
        assert p.returncode == 0, p.stderr[-3000:]
    assert all(p.stdout == runs[0].stdout for p in runs) and len(runs[0].stdout.splitlines()) >= 2
    assert all(messages(p) == messages(runs[0]) for p in runs), [messages(p) for p in runs]
    if command == "profile":
        assert any("% of reads detected in database" in m for m in messages(runs[0]))
    if not seq_id:
        assert any("running median of the counts above 1" in m for m in messages(runs[0]))


def test_the_device_road_is_taken_and_a_declined_summary_falls_back(data):
    d = data["dir"]
    args = ("profile", data["db"], "-c", "50", "-u", "-1", d / "s_1.fq", "-2", d / "s_2.fq")
    host = run(*args, unknown="0", SYLPH_HIP_FEED_TRACE="1")
    dev = run(*args, unknown="1", SYLPH_HIP_FEED_TRACE="1")
    tiny = run(*args, unknown="1", SYLPH_HIP_FEED_TRACE="1", SYLPH_HIP_TABLE_SUMMARY_CAPS="2", SYLPH_HIP_TABLE_SUMMARY_CHUNK="8")
    for p in (host, dev, tiny):
        assert p.returncode == 0, p.stderr[-3000:]
    assert host.stdout == dev.stdout == tiny.stdout and messages(host) == messages(dev) == messages(tiny)
    assert TRACE.findall(host.stderr) == []
    td, tt = TRACE.findall(dev.stderr), TRACE.findall(tiny.stderr)
    assert len(td) == 1 and td[0][1] == "device" and td[0][2] == "0", dev.stderr[-2000:]
    assert len(tt) == 1 and tt[0][1] == "host (declined)" and tt[0][2] == "1", tiny.stderr[-2000:]


@pytest.mark.parametrize("kind", ["raw", "sylsp"])
def test_only_makes_a_declined_summary_an_error_naming_the_file(data, kind):
    """a cap of 2 is reached by every table with two counts above 1 in a row: the real sample declines"""
    args = ("profile", data["db"], "-c", "50", "-u") + samples(data, kind)
    p = run(*args, unknown="only", SYLPH_HIP_TABLE_SUMMARY_CAPS="2", SYLPH_HIP_TABLE_SUMMARY_CHUNK="8")
    first = str(samples(data, kind)[1] if kind == "raw" else samples(data, kind)[0])
    assert p.returncode != 0 and "SYLPH_HIP_UNKNOWN_DEVICE=only" in p.stderr and first in p.stderr and "declined" in p.stderr, p.stderr[-2000:]
    assert run(*args, unknown="only").returncode == 0


def test_a_bad_route_value_fails_before_any_work(data):
    d = data["dir"]
    p = run("query", d / "no_such.syldb", "-c", "50", "-u", "-1", d / "thin_1.fq", "-2", d / "thin_2.fq", unknown="maybe")
    assert p.returncode == 1 and "SYLPH_HIP_UNKNOWN_DEVICE must be 0, 1 or only" in p.stderr and "no_such" not in p.stderr
