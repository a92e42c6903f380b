"""bzip2 streamed through the device decoder one slice at a time (csrc/bunzip2.hip sylph_bunzip2_stream_*, csrc/bunzip2_stream_plan.h)
against Python's bz2 (libbz2): the windows, put together, are libbz2's text byte for byte, or the call fails with SYLPH_ERR_FORMAT having
handed out nothing libbz2 would not have produced before that point.  The matrix is tests/test_bunzip2_stream_plan.py's (the bookkeeping
alone, on the CPU), through the ABI; the texts are tests/bunzip2_stream_inputs.py's: ~1.2 MB of FASTQ (at -1 a dozen blocks of ~22 kB
compressed), 300 kB of noise (at -1 blocks of ~100 kB, each larger than a 64 KiB slice; at -9 one of ~300 kB), run-length edges."""
import bz2

import numpy as np
import pytest

import sylph_amd as S
from sylph_amd.binding import ERR_FORMAT, MEM_DEVICE, SylphHipError

from .bunzip2_stream_inputs import eos_crc_bit, fasta_reads_text, flip, libbz2_prefix, magic_bits, packed, texts

pytestmark = pytest.mark.gpu
KiB = 1024


def drain(ctx, files, slice_kib, order="all", keep="nothing", limit=4000):
    """Runs a stream over `files` to its end the way a consumer would and returns (every file's text, the stream's info).  The slice
    comes from the context's "bunzip2_slice_bytes".  order: "all" = every file advances in every step, "alternate" = one file per step,
    taking turns.  keep: "nothing" = keep_from is NULL, "end" = keep_from = each window's length, "half" = the consumer takes the first
    half of every window and keeps the rest — the kept bytes must reappear at the front of the next window, unchanged."""
    ctx.set_option("bunzip2_slice_bytes", str(slice_kib * KiB))
    st = None
    prev = None
    try:
        st = S.Bunzip2Stream(ctx, files)
        F = len(files)
        out = [bytearray() for _ in range(F)]
        held = [b""] * F                                     # what the consumer kept of the previous window
        keep_from = None
        for step in range(limit):
            if order == "alternate":
                turn = step % F
                if st.finished[turn]:
                    turn = next(i for i in range(F) if not st.finished[i])
                advance = [i == turn for i in range(F)]
            else:
                advance = None
            w = st.next(advance, keep_from)
            if prev is not None:
                prev.close()
            prev = w
            keep_from = []
            for i in range(F):
                got = w.read_file(i)
                assert got[:len(held[i])] == held[i], (i, step)
                if advance is not None and not advance[i]:
                    assert len(got) == len(held[i])          # a file that did not advance gives nothing new
                done = st.finished[i]
                take = len(got) if keep != "half" or done else len(got) // 2
                out[i] += got[:take]
                held[i] = got[take:]
                keep_from.append(take)
            if keep == "nothing":
                assert all(not h for h in held)
                keep_from = None
            if all(st.finished):
                break
        else:
            raise AssertionError("the stream does not end")
        assert all(not h for h in held)
        return [bytes(o) for o in out], st.info()
    finally:
        if prev is not None:
            prev.close()
        if st is not None:
            st.close()
        ctx.set_option("bunzip2_slice_bytes", "0")


@pytest.mark.parametrize("slice_kib", [64, 128, 256])
@pytest.mark.parametrize("level", [1, 9])
def test_the_windows_put_together_are_libbz2s_text(ctx, level, slice_kib):
    t = texts()
    for name in ("fastq", "noise", "runs"):
        data = packed(name, level)
        (got,), info = drain(ctx, [data], slice_kib)
        assert len(got) == len(t[name]) and got == t[name] == bz2.decompress(data), name
        assert info["text_bytes"] == len(got) and info["n_slices"] >= (len(data) // (slice_kib * KiB) if (name, level) == ("fastq", 1) else 1), name


@pytest.mark.parametrize("slice_kib", [64, 128, 256])
@pytest.mark.parametrize("level", [1, 9])
def test_two_files_advancing_together_and_alternately(ctx, level, slice_kib):
    t = texts()
    files = [packed("fastq", level), packed("fastq2", level)]
    for order, keep in (("all", "nothing"), ("alternate", "end")):
        got, info = drain(ctx, files, slice_kib, order=order, keep=keep)
        assert got[0] == t["fastq"] and got[1] == t["fastq2"], order
    # the other mate's bytes lie 256-aligned behind a slice in the upload: a block at a slice's end never reads them
    got, _ = drain(ctx, [packed("noise", 1), packed("fastq2", level)], slice_kib)
    assert got[0] == t["noise"] and got[1] == t["fastq2"]


@pytest.mark.parametrize("order", ["all", "alternate"])
def test_keep_from_in_the_middle_of_the_previous_window(ctx, order):
    t = texts()
    got, info = drain(ctx, [packed("fastq", 1), packed("fastq2", 1)], 64, order=order, keep="half")
    assert got[0] == t["fastq"] and got[1] == t["fastq2"]
    assert info["peak_window_bytes"] < len(t["fastq"]) + len(t["fastq2"])


def test_small_batches_of_candidates(ctx, monkeypatch):
    monkeypatch.setenv("SYLPH_HIP_BUNZIP2_BATCH", "2")         # a slice's chain walked across several batches, both files' in one
    t = texts()
    got, _ = drain(ctx, [packed("fastq", 1), packed("fastq2", 1)], 128)
    assert got[0] == t["fastq"] and got[1] == t["fastq2"]


@pytest.mark.parametrize("delta", [0, -1, 1])
def test_stream_boundary_on_before_and_behind_a_slice_end(ctx, delta):
    t = texts()
    a, b = packed("fastq", 1), packed("fastq2", 1)
    ctx.set_option("bunzip2_slice_bytes", str(len(a) - delta))               # the first slice ends `delta` bytes in front of the stream's end
    st = S.Bunzip2Stream(ctx, [a + b])
    try:
        w = st.next()
        assert w.read_file(0) == t["fastq"] and not st.finished[0]
        w2 = st.next(None, [len(t["fastq"])])
        assert w2.read_file(0) == t["fastq2"] and st.finished[0]
        assert w.n_members + w2.n_members == 2 and w.n_blocks + w2.n_blocks == len(magic_bits(a + b))
        w.close(); w2.close()
    finally:
        st.close()
        ctx.set_option("bunzip2_slice_bytes", "0")


def test_empty_streams_between_others_and_a_stream_over_three_slices(ctx):
    t = texts()
    data = packed("fastq2", 9) + bz2.compress(b"", 9) + packed("fastq", 1) + bz2.compress(b"", 1) + bz2.compress(b"", 1) + packed("noise", 1)
    assert len(packed("fastq", 1)) > 3 * 64 * KiB
    (got,), info = drain(ctx, [data], 64)
    assert got == t["fastq2"] + t["fastq"] + t["noise"] and info["n_slices"] >= 6
    (got,), info = drain(ctx, [bz2.compress(b"", 9)], 64)
    assert got == b"" and info["n_slices"] == 1


def _sketch(ctx, push, paired=False):
    sk = S.ReadSketcher(ctx, c=5, paired=paired)
    try:
        push(sk)
        return sk.finish()
    finally:
        sk.close()


def _records(text, fasta):
    lines = text.split(b"\n")[:-1]
    seqs = lines[1::2] if fasta else lines[1::4]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), off


@pytest.mark.parametrize("kind", ["fastq", "fasta", "pair"])
def test_every_window_indexed_and_pushed_equals_the_array_push(ctx, kind):
    from .test_gpu_parity import assert_same_sketch
    t = texts()
    fasta = kind == "fasta"
    plain = [fasta_reads_text(np.random.default_rng(5), 4000)] if fasta else [t["fastq"]] + ([t["fastq2"]] if kind == "pair" else [])
    Index = S.FastaText if fasta else S.FastqText
    F = len(plain)

    def streamed(sk):
        ctx.set_option("bunzip2_slice_bytes", str(64 * KiB))
        st = S.Bunzip2Stream(ctx, [bz2.compress(p, 1) for p in plain])
        prev, keep, advance, pushed = None, None, None, 0
        try:
            for _ in range(1000):
                w = st.next(advance, keep)
                if prev is not None:
                    prev.close()
                prev = w
                idx = [Index(ctx, w.files[i][0], MEM_DEVICE, w.files[i][1], final=int(st.finished[i])) if w.files[i][1] else None for i in range(F)]
                n = min(x.n_records if x else 0 for x in idx)
                if n:
                    (sk.push_fasta if fasta else sk.push_fastq)(idx[0], idx[1] if F == 2 else None, 0, n)
                    pushed += n
                keep = [min(x.record_offset(n), w.files[i][1]) if x else 0 for i, x in enumerate(idx)]
                waiting = [(x.n_records if x else 0) - n for x in idx]
                for x in idx:
                    if x:
                        x.close()
                if all(st.finished) or any(st.finished[i] and waiting[i] == 0 for i in range(F)):
                    break
                advance = [not st.finished[i] and (waiting[i] <= min(waiting) or st.finished[1 - i] if F == 2 else True) for i in range(F)]
            else:
                raise AssertionError("the stream does not end")
            assert st.info()["n_slices"] >= 3
            return pushed
        finally:
            if prev is not None:
                prev.close()
            st.close()
            ctx.set_option("bunzip2_slice_bytes", "0")

    counts = {}
    got = _sketch(ctx, lambda sk: counts.setdefault("n", streamed(sk)), paired=F == 2)
    if F == 1:
        bases, off = _records(plain[0], fasta)
        assert counts["n"] == len(off) - 1
        want = _sketch(ctx, lambda sk: sk.push(bases, off))
    else:
        whole = [S.FastqText(ctx, p) for p in plain]
        assert counts["n"] == min(x.n_records for x in whole)
        want = _sketch(ctx, lambda sk: sk.push_fastq(whole[0], whole[1]), paired=True)
        for x in whole:
            x.close()
    assert len(want["kmers"]) > 1000
    assert_same_sketch(got, want, kind)


def test_the_whole_file_road_declines_at_its_limit_and_the_stream_takes_the_file(ctx):
    """"bunzip2_whole_max_bytes" gives the whole-file road a limit (none by default) for the tests; the stream has none"""
    t = texts()
    data = packed("fastq", 1)
    ctx.set_option("bunzip2_whole_max_bytes", str(len(data)))
    try:
        with pytest.raises(SylphHipError) as ei:
            S.Bunzipped(ctx, data)
        assert ei.value.code == ERR_FORMAT
        with pytest.raises(SylphHipError) as ei:
            S.Bunzipped(ctx, [packed("fastq2", 1), packed("fastq2", 9)])     # all files of the call together
        assert ei.value.code == ERR_FORMAT
        small = S.Bunzipped(ctx, packed("fastq2", 1))                        # below the limit: as ever
        assert small.read().tobytes() == t["fastq2"]
        small.close()
        (got,), _ = drain(ctx, [data], 128)
        assert got == t["fastq"]
    finally:
        ctx.set_option("bunzip2_whole_max_bytes", "0")
    whole = S.Bunzipped(ctx, data)
    assert whole.n_bytes == len(t["fastq"])
    whole.close()
    with pytest.raises(SylphHipError):
        ctx.set_option("bunzip2_slice_bytes", "1000")                        # a slice is 64 KiB at least


def test_scratch_is_a_function_of_the_slice_not_of_the_file(ctx):
    """K9b's condition, a guard: the short file is longer than a slice and its overlap already (five streams, 1.3 MB compressed), the long
    one four times that; both upload 64 KiB + 1 MiB per call."""
    t = texts()
    short = packed("fastq", 1) * 5
    long_ = short * 4
    assert len(short) > 64 * KiB + (1 << 20)
    (got,), a = drain(ctx, [short], 64)
    assert got == t["fastq"] * 5
    (got,), b = drain(ctx, [long_], 64)
    assert got == t["fastq"] * 20 and b["n_slices"] >= 3 * a["n_slices"]
    assert a["peak_scratch_bytes"] > 0 and b["peak_scratch_bytes"] <= 1.5 * a["peak_scratch_bytes"]
    assert b["peak_window_bytes"] <= 2 * a["peak_window_bytes"]


def test_damage_is_err_format_from_the_next_that_holds_it_and_the_context_is_fine_afterwards(ctx):
    """files that fail; none of them makes a kernel fault"""
    t = texts()
    text, good = t["fastq"], packed("fastq", 1)
    bits = magic_bits(good)
    assert len(bits) >= 10 and bits[8] // 8 > 2 * 64 * KiB                  # block 8 lies behind two slices
    st = S.Bunzip2Stream(ctx, [good], 64 * KiB)
    ends, prev = [], None                                  # text bytes after every slice of the good file
    while not st.finished[0]:
        w = st.next()
        if prev is not None:
            prev.close()
        prev = w
        ends.append((ends[-1] if ends else 0) + w.files[0][1])
    prev.close()
    st.close()
    assert len(ends) >= 3 and ends[-1] == len(text)
    randomised = bytearray(good)
    mid = (bits[8] + bits[9]) // 16
    randomised[mid:mid + 2000] = np.random.default_rng(3).integers(0, 256, size=2000, dtype=np.uint8).tobytes()
    cases = {"symbol bit in a late block": (flip(good, (bits[8] + bits[9]) // 2), ends[1]), "block crc": (flip(good, bits[8] + 48 + 5), ends[1]),
             "stream crc": (flip(good, eos_crc_bit(good) + 7), ends[-2]), "truncated": (good[:-30], ends[-2]), "cut in half": (good[:len(good) // 2], ends[0]),
             "a randomised block": (bytes(randomised), ends[1]), "the randomised bit": (flip(good, bits[8] + 80), ends[1]), "trailing bytes": (good + b"not bzip2", ends[-2])}
    for name, (bad, at_least) in cases.items():
        st = S.Bunzip2Stream(ctx, [bad], 64 * KiB)
        got, prev = bytearray(), None
        with pytest.raises(SylphHipError) as ei:
            for _ in range(len(ends) + 2):
                w = st.next()
                if prev is not None:
                    prev.close()
                prev = w
                got += w.read_file(0)
            raise AssertionError("not declined: " + name)
        if prev is not None:
            prev.close()
        assert ei.value.code == ERR_FORMAT, (name, str(ei.value))
        assert len(got) >= at_least, name                                    # declined by the `next` that holds the damage, not before
        assert len(got) < len(text) or name in ("stream crc", "trailing bytes"), name
        lib = libbz2_prefix(bad)
        assert lib[:len(got)] == bytes(got) and len(lib) >= len(got), name   # never a byte libbz2 would not have produced before that point
        with pytest.raises(SylphHipError) as ei:                             # the stream is dead
            st.next()
        assert ei.value.code == ERR_FORMAT
        st.close()
        # a fresh stream on a good file works afterwards, and so does the whole-file road
        (again,), _ = drain(ctx, [packed("fastq2", 1)], 64)
        assert again == t["fastq2"], name
    whole = S.Bunzipped(ctx, good)
    assert whole.read().tobytes() == text
    whole.close()
    for not_bzip2 in (b"BZh0" + good[4:], b"\x1f\x8b" + good[2:]):
        with pytest.raises(SylphHipError) as ei:
            S.Bunzip2Stream(ctx, [good, not_bzip2], 64 * KiB)
        assert ei.value.code == ERR_FORMAT
