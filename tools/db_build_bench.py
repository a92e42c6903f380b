"""`sylph-hip sketch` of a directory of genome files (FASTA, half of them gzip): wall time of the database build.
  python tools/db_build_bench.py [n_files]                     -t 1, 8 and 32; the database must not depend on -t
  python tools/db_build_bench.py [n_files] --roads [-t 16] [--runs 3]
                                                               the genome files' device road (csrc/fasta.hip, SYLPH_HIP_FASTA_DEVICE=1) against the host
                                                               road (SYLPH_HIP_FASTA_DEVICE=0), alternating, `runs` runs each: medians,
                                                               spread, and the two databases compared byte for byte
GPU box."""
import argparse, gzip, os, subprocess, sys, tempfile, time
from concurrent.futures import ProcessPoolExecutor
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLEN = 4_000_000


def write_genome(job):
    d, i = job
    rng = np.random.default_rng([3, i])
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=GLEN)]
    lines = [b">g%d contig_1 synthetic" % i] + [seq[j:j + 80].tobytes() for j in range(0, GLEN, 80)]
    p = os.path.join(d, f"g{i}.fa.gz" if i % 2 else f"g{i}.fa")
    data = b"\n".join(lines) + b"\n"
    if i % 2:
        with gzip.open(p, "wb", compresslevel=1) as f:
            f.write(data)
    else:
        open(p, "wb").write(data)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_files", nargs="?", type=int, default=160)
    ap.add_argument("--roads", action="store_true")
    ap.add_argument("-t", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix="sylph_db_")
    t = time.time()
    with ProcessPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        paths = list(ex.map(write_genome, [(d, i) for i in range(a.n_files)]))
    lst = os.path.join(d, "genomes.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    print(f"{a.n_files} genome files of {GLEN / 1e6:.0f} Mbp (half of them gzip) written in {time.time() - t:.1f} s", flush=True)
    exe = os.path.join(ROOT, "sylph_amd", "sylph-hip")
    gbp = a.n_files * GLEN / 1e9

    def build(out, threads, env_extra):
        env = dict(os.environ)
        env.pop("SYLPH_HIP_FASTA_DEVICE", None)
        env.update(env_extra)
        t = time.time()
        r = subprocess.run([exe, "sketch", "-l", lst, "-o", out, "-t", str(threads)], capture_output=True, text=True, env=env)
        dt = time.time() - t
        assert r.returncode == 0, r.stderr[-2000:]
        return dt, open(out + ".syldb", "rb").read(), r.stderr

    if a.roads:
        roads = (("host road (SYLPH_HIP_FASTA_DEVICE=0)", {"SYLPH_HIP_FASTA_DEVICE": "0"}), ("device road (SYLPH_HIP_FASTA_DEVICE=1)", {"SYLPH_HIP_FASTA_DEVICE": "1"}))
        times, dbs = {name: [] for name, _ in roads}, {}
        build(os.path.join(d, "warm"), a.t, roads[1][1])                      # (page cache, GPU runtime's caches: not counted)
        for run in range(a.runs):
            for name, env in roads:
                device = env["SYLPH_HIP_FASTA_DEVICE"] == "1"
                dt, db, err = build(os.path.join(d, f"db_{len(times[name])}_{'d' if device else 'h'}"), a.t, dict(env, SYLPH_HIP_FEED_TRACE="1"))
                times[name].append(dt)
                dbs[name] = db
                laps = [ln.split() for ln in err.splitlines() if "genomes fasta-device" in ln]
                declined = sum(int(w[5].split("=")[1]) for w in laps)
                in_windows = sum(float(w[6]) for w in laps) / 1e3
                print(f"run {run} {name}: {dt:.2f} s = {gbp / dt:.2f} Gbp/s" +
                      (f" ({len(laps)} windows of files: {in_windows:.2f} s in them; files declined by the device: {declined})" if device else ""), flush=True)
        for name, _ in roads:
            v = sorted(times[name])
            print(f"{name}, -t {a.t}, {a.runs} runs: median {np.median(v):.2f} s = {gbp / np.median(v):.2f} Gbp/s, min {v[0]:.2f} s, max {v[-1]:.2f} s, spread {v[-1] - v[0]:.2f} s")
        assert dbs[roads[0][0]] == dbs[roads[1][0]], "the two roads must write the same database"
        print("databases of the two roads identical")
        return
    res = {}
    for threads in (1, 8, 32):
        dt, res[threads], _ = build(os.path.join(d, f"db_t{threads}"), threads, {})
        print(f"-t {threads}: {dt:.2f} s = {gbp / dt:.2f} Gbp/s (database {len(res[threads]) / 1e6:.1f} MB)")
    assert res[1] == res[8] == res[32], "the database must not depend on -t"
    print("databases identical for every -t")


if __name__ == "__main__":
    main()
