"""GPU tests of a pre-sketched sample's table made on the device (csrc/sylsp.hip): sylph_table_from_entries / sylph_table_view
against the host's read_sylsp on the same bytes and against the numpy model (stable argsort by key, last of each run), bit for bit,
over every tile shape, order and alignment; and sylph_pipeline_submit_entries — such samples through the pipeline, beside raw
ones, in submission order, over one database and over two replicas."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import sylph_amd as S
from oracle import oracle as O
from sylph_amd.binding import MEM_DEVICE, MEM_HOST

from .sylsp_tables import CASE_KINDS, MANY, SIZES, entries_case, model_table, pack_entries
from .test_gpu_pipeline import check_result, sample_reads, small_world

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_SIZES = SIZES + [MANY]


def d2h(ptr, n, dtype):
    """n items of device memory (the runtime the library itself is linked against does the copy)"""
    out = np.zeros(n, dtype=dtype)
    if n:
        memcpy = S.load().hipMemcpy
        memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert memcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0              # hipMemcpyDeviceToHost
    return out


def table_arrays(t):
    return d2h(t.dev_kmers, t.n, np.uint64), d2h(t.dev_counts, t.n, np.uint32)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """(kind, n) -> entries, their packed bytes, the model's table — and the host reader's table of the same bytes in a .sylsp file,
    which must be the model's.  Made once for the module; nobody writes to them."""
    H = C.CDLL(os.path.join(ROOT, "sylph_amd", "libsylph_host.so"))
    H.sylph_host_read_sylsp.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 5 + [C.c_char_p, C.c_char_p, C.c_uint64, C.c_void_p]
    d = tmp_path_factory.mktemp("sylsp")
    out = {}
    for kind in CASE_KINDS:
        for n in ALL_SIZES:
            kmers, counts = entries_case(kind, n)
            raw = pack_entries(kmers, counts)
            want_k, want_c = model_table(kmers, counts)
            p = d / f"{kind}_{n}.sylsp"
            tail = struct.pack("<QQQ", 200, 31, 1) + b"x" + b"\x00\x01" + struct.pack("<d", 150.0)
            p.write_bytes(struct.pack("<Q", n) + raw.tobytes() + tail)
            hk, hc = np.zeros(max(1, n), dtype=np.uint64), np.zeros(max(1, n), dtype=np.uint32)
            m, c, k, pr, hs, mean = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int(), C.c_int(), C.c_double()
            fn, sn = C.create_string_buffer(64), C.create_string_buffer(64)
            assert H.sylph_host_read_sylsp(str(p).encode(), hk.ctypes.data, hc.ctypes.data, max(1, n), C.byref(m), C.byref(c), C.byref(k), C.byref(pr),
                                           C.byref(mean), fn, sn, 64, C.byref(hs)) == 0
            assert np.array_equal(hk[:m.value], want_k) and np.array_equal(hc[:m.value], want_c)
            ascending = n < 2 or bool((kmers[1:] > kmers[:-1]).all())
            for a in (kmers, counts, raw, want_k, want_c):
                a.setflags(write=False)
            out[(kind, n)] = (kmers, counts, raw, want_k, want_c, ascending)
    assert not out[("permutation", MANY)][5] and len(out[("duplicates", MANY)][3]) < MANY
    return out


def launches(ctx, family):
    return ctx.kernel_stats(family)[1]


@pytest.mark.parametrize("kind", CASE_KINDS)
def test_table_from_host_entries_at_every_alignment(ctx, cases, kind):
    """Host entries 0 to 3 bytes off an aligned address: the table is the host reader's and the model's, bit for bit; entries
    that ascend strictly are unpacked by ONE launch and nothing is sorted (the kernel timers' launch counts)."""
    ctx.profile(True)
    try:
        for n in ALL_SIZES:
            kmers, counts, raw, want_k, want_c, ascending = cases[(kind, n)]
            for shift in range(4):
                buf = np.zeros(len(raw) + 16, dtype=np.uint8)
                shift_now = (-buf.ctypes.data) % 8 + shift                  # `shift` bytes off an 8-byte boundary
                src = buf[shift_now:shift_now + len(raw)]
                src[:] = raw
                assert n == 0 or src.ctypes.data % 4 == shift % 4
                before = {f: launches(ctx, f) for f in ("sylsp", "sort", "sylsp_dedup")}
                t = S.Table(ctx, src, n_entries=n)
                after = {f: launches(ctx, f) for f in ("sylsp", "sort", "sylsp_dedup")}
                got_k, got_c = table_arrays(t)
                assert t.was_ascending == ascending and t.n == len(want_k), (n, shift)
                assert np.array_equal(got_k, want_k) and np.array_equal(got_c, want_c), (n, shift)
                delta = {f: after[f] - before[f] for f in after}
                assert delta == {"sylsp": int(n > 0), "sort": int(not ascending), "sylsp_dedup": int(not ascending)}, (n, shift, delta)
                t.close()
    finally:
        ctx.profile(False)


@pytest.mark.parametrize("kind", CASE_KINDS)
def test_table_from_device_entries_at_every_phase(ctx, cases, kind):
    """Borrowed device entries 0 to 3 dwords behind a 16-byte boundary, 16 readable bytes either side (filled with 0xFF: nothing may
    depend on them); the input is left as it was."""
    import torch
    for n in ALL_SIZES:
        kmers, counts, raw, want_k, want_c, ascending = cases[(kind, n)]
        for phase in range(4):
            lead = 16 + 4 * phase
            host = np.full(lead + len(raw) + 16, 0xFF, dtype=np.uint8)
            host[lead:lead + len(raw)] = raw
            dev = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
            assert dev.data_ptr() % 16 == 0
            t = S.Table(ctx, dev.data_ptr() + lead, n_entries=n, mem=MEM_DEVICE)
            got_k, got_c = table_arrays(t)
            assert t.was_ascending == ascending and t.n == len(want_k), (n, phase)
            assert np.array_equal(got_k, want_k) and np.array_equal(got_c, want_c), (n, phase)
            assert np.array_equal(dev.cpu().numpy(), host)
            t.close()


def test_table_refusals_leave_the_context_usable(ctx, cases):
    import torch
    kmers, counts, raw, want_k, want_c, _ = cases[("duplicates", 257)]
    dev = torch.from_numpy(np.concatenate([np.zeros(16, np.uint8), raw, np.zeros(16, np.uint8)])).cuda()
    torch.cuda.synchronize()
    for off in (1, 2, 3):                                                    # a device pointer that is not 4-byte aligned
        with pytest.raises(S.SylphHipError) as e:
            S.Table(ctx, dev.data_ptr() + 16 + off, n_entries=10, mem=MEM_DEVICE)
        assert e.value.code == -1 and "4-byte aligned" in str(e.value)
    tiny = np.zeros(12, dtype=np.uint8)
    for mem, ptr in ((MEM_HOST, tiny), (MEM_DEVICE, dev.data_ptr() + 16)):   # 2^31 entries: refused before a byte of them is read
        with pytest.raises(S.SylphHipError) as e:
            S.Table(ctx, ptr, n_entries=2**31, mem=mem)
        assert e.value.code == -1 and "2^31" in str(e.value)
    with pytest.raises(S.SylphHipError):
        S.Table(ctx, 0, n_entries=5, mem=MEM_DEVICE)                         # null entries
    t = S.Table(ctx, dev.data_ptr() + 16, n_entries=257, mem=MEM_DEVICE)
    got_k, got_c = table_arrays(t)
    assert np.array_equal(got_k, want_k) and np.array_equal(got_c, want_c) and not t.was_ascending
    t.close()


def test_table_goes_where_a_device_table_goes(ctx):
    """The view's pointers under MEM_DEVICE: sylph_db_contain and sylph_db_contain_view give what the host table gives."""
    rng, genomes, db_k, goff = small_world(31)
    db = S.Database(ctx, db_k, goff)
    kmers, counts = sample_table(rng, db_k, goff, 2, "duplicates")
    want_k, want_c = model_table(kmers, counts)
    t = S.Table(ctx, pack_entries(kmers, counts))
    cc0, off0, covs0 = db.contain(want_k, want_c)
    cc1, off1, covs1 = db.contain(t.dev_kmers, t.dev_counts, device_ptrs=True, n=t.n)
    assert cc0.max() > 0 and np.array_equal(cc0, cc1) and np.array_equal(off0, off1) and np.array_equal(covs0, covs1)
    cc2, off2, covs2 = db.contain_view(t.dev_kmers, t.dev_counts, device_ptrs=True, n=t.n)
    assert np.array_equal(cc0, cc2) and np.array_equal(off0, off2) and np.array_equal(covs0, covs2)
    t.close()
    db.close()


# ---- through the pipeline ----------------------------------------------------------------------------------------------------

def sample_table(rng, db_k, goff, g, kind):
    """the entries of a sample that holds most of genome g's k-mers and some nobody has; one database k-mer with a count of 0"""
    mine = db_k[int(goff[g]):int(goff[g + 1])]
    held = mine[rng.random(len(mine)) < 0.7]
    kmers = np.unique(np.concatenate([held, rng.integers(1, 2**63, size=300, dtype=np.uint64)]))
    counts = rng.integers(1, 60, size=len(kmers)).astype(np.uint32)
    counts[np.searchsorted(kmers, held[len(held) // 2])] = 0
    if kind == "ascending":
        return kmers, counts
    perm = rng.permutation(len(kmers))
    kmers, counts = kmers[perm], counts[perm]
    if kind == "duplicates":
        dst = rng.choice(len(kmers), size=len(kmers) // 100, replace=False)
        kmers[dst] = kmers[(dst + 7) % len(kmers)]
    return kmers, counts


def expected_rows(db, tables):
    out = []
    for kmers, counts in tables:
        wk, wc = model_table(kmers, counts)
        cc, off, covs = db.contain_view(wk, wc)
        out.append((wk, wc, cc.copy(), off.copy(), np.asarray(covs).astype(np.uint32).copy()))
    return out


def check_entries_result(r, want, G):
    wk, wc, cc, off, covs = want
    assert r["n_table"] == len(wk) and r["dup_removed"] == 0
    assert np.array_equal(r["kmers"], wk) and np.array_equal(r["counts"], wc)          # want_table
    assert np.array_equal(r["contain_count"], cc)
    ro, rc = r["cov_off"], np.asarray(r["covs"]).astype(np.uint32)
    for g in range(G):                                                                # (a batch's samples share `covs`: through cov_off)
        assert np.array_equal(rc[int(ro[g]):int(ro[g + 1])], covs[int(off[g]):int(off[g + 1])]), g
    t = r["t"]
    assert t[0] <= t[1] <= t[2] <= t[3] <= t[4]


def test_pipeline_entries_beside_read_batches_in_submission_order(ctx):
    import torch
    rng, genomes, db_k, goff = small_world(41)
    G = len(goff) - 1
    db = S.Database(ctx, db_k, goff)
    kinds = ["ascending", "permutation", "duplicates", "ascending", "duplicates", "permutation"]
    tables = [sample_table(rng, db_k, goff, i % G, kind) for i, kind in enumerate(kinds)]
    want = expected_rows(db, tables)
    assert all(w[2].max() > 50 for w in want)
    raws = [pack_entries(k, c) for k, c in tables]
    devs = [torch.from_numpy(np.concatenate([np.zeros(16, np.uint8), r, np.zeros(16, np.uint8)])).cuda() for r in raws]
    torch.cuda.synchronize()
    reads = [sample_reads(rng, genomes, [i], 400) for i in (1, 3)]
    reads_want = [O.sketch_reads(b, off, c=50, paired=True) for b, off in reads]
    for workers, depth, max_batch in ((1, 2, 1), (2, 9, 4)):
        p = S.Pipeline(db, c=50, paired=True, n_workers=workers, depth=depth, max_batch=max_batch, want_table=True)
        plan = []                                                            # ("entries", i) | ("reads", i) | ("empty", None)
        for i in range(len(tables)):
            plan.append(("entries", i))
            if i in (1, 4):
                plan.append(("reads", len([x for x in plan if x[0] == "reads"])))
            if i == 2:
                plan.append(("empty", None))
        submitted = done = 0
        while done < len(plan):
            while submitted < len(plan) and p.outstanding < depth:
                what, i = plan[submitted]
                if what == "entries" and i % 2 == 0:
                    ok = p.submit_entries(raws[i].ctypes.data, len(tables[i][0]), tag=submitted)
                elif what == "entries":
                    ok = p.submit_entries(devs[i].data_ptr() + 16, len(tables[i][0]), tag=submitted, mem=MEM_DEVICE)
                elif what == "empty":
                    ok = p.submit_entries(None, 0, tag=submitted)
                else:
                    b, off = reads[i]
                    ok = p.submit_device([(b.ctypes.data, off.ctypes.data, len(off) - 1, int(off[-1]))], tag=submitted, mem=MEM_HOST)
                assert ok
                submitted += 1
            if submitted < len(plan) and plan[submitted][0] == "entries":    # depth reached: refused, not blocked
                assert p.submit_entries(raws[0].ctypes.data, len(tables[0][0])) is False
            r = p.next()
            assert r["tag"] == done                                          # submission order
            what, i = plan[done]
            if what == "entries":
                check_entries_result(r, want[i], G)
                assert p.ascending_of_last() == int(kinds[i] == "ascending")
            elif what == "empty":
                assert r["n_table"] == 0 and r["dup_removed"] == 0 and not r["contain_count"].any() and p.ascending_of_last() == 1
                assert len(r["kmers"]) == 0 and int(r["cov_off"][G]) == int(r["cov_off"][0])
            else:
                check_result(r, reads_want[i], db_k, goff)
                assert p.ascending_of_last() == -1
            assert 1 <= r["probe_batch"] <= max_batch
            done += 1
        with pytest.raises(S.SylphHipError):
            p.next()
        p.close()
    db.close()


def test_pipeline_entries_over_two_replicas_sharing_the_gpu(ctx):
    import torch
    rng, genomes, db_k, goff = small_world(43)
    G = len(goff) - 1
    db = S.Database(ctx, db_k, goff)
    ctx2 = S.Context(0)
    reps = [db, db.replicate(ctx2)]
    kinds = ["permutation", "ascending", "duplicates", "ascending", "permutation", "duplicates", "ascending"]
    tables = [sample_table(rng, db_k, goff, (2 * i) % G, kind) for i, kind in enumerate(kinds)]
    want = expected_rows(db, tables)
    raws = [pack_entries(k, c) for k, c in tables]
    devs = [torch.from_numpy(np.concatenate([np.zeros(16, np.uint8), r, np.zeros(16, np.uint8)])).cuda() for r in raws]
    torch.cuda.synchronize()
    p = S.Pipeline(reps, c=50, paired=True, n_workers=2, depth=3, max_batch=4, want_table=True)
    def submit(i):                                                           # host memory: the least busy replica; device memory: one on that device
        if i % 2 == 0:
            return p.submit_entries(raws[i].ctypes.data, len(tables[i][0]), tag=i)
        return p.submit_entries(devs[i].data_ptr() + 16, len(tables[i][0]), tag=i, mem=MEM_DEVICE)
    for i in range(6):
        assert submit(i)
    assert submit(6) is False                                                # 2 replicas x depth 3 outstanding: refused, not blocked
    used = set()
    for i in range(len(tables)):
        r = p.next()
        assert r["tag"] == i
        used.add(r["replica"])
        check_entries_result(r, want[i], G)
        assert p.ascending_of_last() == int(kinds[i] == "ascending")
        if i == 0:
            assert submit(6)
    assert used == {0, 1}
    p.close()
    reps[1].close()
    ctx2.close()
    db.close()
