"""GPU tests of `sylph-hip profile` / `query` with the first pass's statistics head counted on the device (SYLPH_HIP_STATS_DEVICE=only:
the pipeline hands over the candidate rows only, csrc/row_stats.hip) against the host's walk over every row with a hit (=0) and the
default: the same bytes on stdout, the same reassignment log.  Inputs are tests/test_gpu_cli_bootstrap.py's: three E. coli slices and
an unrelated genome, reads at full and at thinned coverage (a lambda and an interval are estimated there); the same reads as sketch
files take the pipeline's other road."""
import os
import re
import subprocess

import pytest

from .test_gpu_cli_bootstrap import build_inputs, ci_columns

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sylph_amd", "sylph-hip")
TRACE = re.compile(r"^\[sylph_hip feed\] stats (\S+): road (\w+), (?:(\d+) rows with hits, )?(\d+) candidates$", re.M)


def run(*args, stats=None, **env):
    e = dict(os.environ, SYLPH_HIP_EXACT_DEDUP="1", **env)
    e.pop("SYLPH_HIP_STATS_DEVICE", None)
    if stats is not None:
        e["SYLPH_HIP_STATS_DEVICE"] = stats
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=e)


@pytest.fixture(scope="module")
def data(tmp_path_factory, golden_dir):
    d = build_inputs(tmp_path_factory.mktemp("cli_row_stats"), golden_dir)
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
        return [tuple(data["sylsp"])]
    return [("-1", d / f"{reads}_1.fq", "-2", d / f"{reads}_2.fq") for reads in ("s", "thin")]


FLAGS = {"plain": (), "u": ("-u",), "no_ci": ("--no-ci",), "m80": ("-m", "80"), "no_adjust": ("--no-adjust",)}


@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("kind", ["raw", "sylsp"])
@pytest.mark.parametrize("command", ["profile", "query"])
def test_device_road_prints_the_hosts_bytes(data, command, kind, flags):
    """stdout for SYLPH_HIP_STATS_DEVICE = 0 and only — and, for the plain command, unset — byte for byte.  The plain command runs every
    sample, a flag the last one (the thinned reads are in it)."""
    all_samples = samples(data, kind)
    rows_with_ci = 0
    for sample in all_samples if flags == "plain" else all_samples[-1:]:
        args = (command, data["db"], "-c", "50") + sample + FLAGS[flags]
        runs = [run(*args, stats="0"), run(*args, stats="only")] + ([run(*args)] if flags == "plain" else [])
        for p in runs:
            assert p.returncode == 0, p.stderr[-3000:]
        assert all(p.stdout == runs[0].stdout for p in runs) and len(runs[0].stdout.splitlines()) >= 2
        rows_with_ci += sum(1 for a, l in ci_columns(runs[0].stdout, command) if a != "NA-NA" and l != "NA-NA")
    assert rows_with_ci >= 1 or flags != "plain"                           # at least one row with a confidence interval


def test_reassignment_log_is_the_same(data):
    def log(p):
        return [l for l in p.stderr.split("\n") if re.search(r"Logging k-mer reassignments|\] Index\t|\] \d+->\d+\t| after reassigning | has ANI ", l)]
    for sample in samples(data, "raw") + samples(data, "sylsp"):
        args = ("profile", data["db"], "-c", "50") + sample + ("--log-reassignments",)
        host, dev = run(*args, stats="0"), run(*args, stats="only")
        assert host.returncode == 0 and dev.returncode == 0, (host.stderr[-2000:], dev.stderr[-2000:])
        assert host.stdout == dev.stdout and log(host) == log(dev) and len(log(host)) >= 3


@pytest.mark.parametrize("command", ["profile", "query"])
def test_trace_shows_fewer_candidates_than_rows_with_hits(data, command):
    """-m 99.5: the strain the reads were not drawn from shares most of its k-mers with them and still falls below the cut — a row with
    hits that is no candidate.  The device's road brings only the candidates to the host, so the rows with hits are the host road's."""
    d = data["dir"]
    args = (command, data["db"], "-c", "50", "-m", "99.5", "-1", d / "s_1.fq", "-2", d / "s_2.fq")
    host, dev = run(*args, stats="0", SYLPH_HIP_FEED_TRACE="1"), run(*args, stats="1", SYLPH_HIP_FEED_TRACE="1")
    assert host.returncode == 0 and dev.returncode == 0 and host.stdout == dev.stdout
    th, td = TRACE.findall(host.stderr), TRACE.findall(dev.stderr)
    assert len(th) == 1 and len(td) == 1, (host.stderr[-2000:], dev.stderr[-2000:])
    assert th[0][1] == "host" and td[0][1] == "device" and th[0][2] != "" and td[0][2] == ""
    assert int(td[0][3]) < int(th[0][2]), (th, td)


def test_a_bad_route_value_is_an_error(data):
    d = data["dir"]
    p = run("query", data["db"], "-c", "50", "-1", d / "thin_1.fq", "-2", d / "thin_2.fq", stats="maybe")
    assert p.returncode == 1 and "SYLPH_HIP_STATS_DEVICE" in p.stderr
