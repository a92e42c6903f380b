"""gzip streamed through the device inflate one slice at a time (csrc/inflate.hip sylph_inflate_stream_*, csrc/inflate_stream_plan.h)
against zlib: the windows, put together, are zlib's text byte for byte, or the call fails with SYLPH_ERR_FORMAT — and the records of
a window found on the device (sylph_fastq_index_window) against a Python split.  The texts are those of tests/test_inflate_plan.py
(deflate blocks of 25-32 KB of compressed bytes: a slice of 128 KiB holds about four).  The bookkeeping alone is tested on the CPU in
tests/test_inflate_stream_plan.py."""
import zlib

import numpy as np
import pytest

import sylph_amd as S
from sylph_amd.binding import ERR_FORMAT, MEM_DEVICE, SylphHipError

from .helpers import bgzf_compress
from .test_inflate_plan import fastq_text, gz_level

pytestmark = pytest.mark.gpu
KiB = 1024


@pytest.fixture(scope="module")
def texts():
    return {level: fastq_text(np.random.default_rng(level), 12000) for level in (1, 6, 9)}      # 3.19 MB each


@pytest.fixture(scope="module")
def gzs(texts):
    return {level: gz_level(t, level) for level, t in texts.items()}


def drain(ctx, files, slice_kib, order="all", keep="nothing", limit=4000):
    """Runs a stream over `files` to its end the way a consumer would and returns (every file's text, the stream's info).  The slice
    comes from the context's "inflate_slice_bytes".  order: "all" = every file advances in every step, "alternate" = one file per step,
    taking turns.  keep: "nothing" = keep_from is NULL, "end" = keep_from = each window's length, "half" = the consumer takes the first
    half of every window and keeps the rest — the kept bytes must reappear at the front of the next window, unchanged."""
    ctx.set_option("inflate_slice_bytes", str(slice_kib * KiB))
    st = None
    prev = None
    try:
        st = S.InflateStream(ctx, files)
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
        ctx.set_option("inflate_slice_bytes", "0")


@pytest.mark.parametrize("slice_kib", [64, 128, 256])
@pytest.mark.parametrize("level", [1, 6, 9])
def test_the_windows_put_together_are_zlibs_text(ctx, texts, gzs, level, slice_kib):
    (got,), info = drain(ctx, [gzs[level]], slice_kib)
    assert got == zlib.decompress(gzs[level], 31) == texts[level]
    assert info["n_slices"] > 1 and info["text_bytes"] == len(got)
    assert info["n_slices"] >= len(gzs[level]) // ((slice_kib + slice_kib // 2) * KiB)


@pytest.mark.parametrize("slice_kib", [64, 128, 256])
def test_two_files_in_one_stream(ctx, texts, gzs, slice_kib):
    got, info = drain(ctx, [gzs[1], gzs[9]], slice_kib)
    assert got[0] == texts[1] and got[1] == texts[9] and info["n_slices"] > 2


@pytest.mark.parametrize("slice_kib", [64, 256])
def test_advance_alternating_between_the_files(ctx, texts, gzs, slice_kib):
    got, info = drain(ctx, [gzs[6], gzs[1]], slice_kib, order="alternate", keep="end")
    assert got[0] == texts[6] and got[1] == texts[1] and info["n_slices"] > 2


@pytest.mark.parametrize("order", ["all", "alternate"])
def test_keep_from_in_the_middle_of_the_previous_window(ctx, texts, gzs, order):
    got, info = drain(ctx, [gzs[6], gzs[9]], 128, order=order, keep="half")
    assert got[0] == texts[6] and got[1] == texts[9]
    assert info["peak_window_bytes"] < len(texts[6]) + len(texts[9])


def test_a_back_reference_that_crosses_the_cut(ctx):
    """30 kB of noise twice: the second copy is matches at distance 30000, a block starts inside the first copy (a block of literals holds
    16 Ki symbols), and at 64 KiB and 96 KiB a cut falls on such a block (tests/test_inflate_stream_plan.py places it with the model)."""
    rng = np.random.default_rng(11)
    half = rng.integers(0, 256, size=30000, dtype=np.uint8).tobytes()
    text = fastq_text(rng, 1100) + half + half + fastq_text(rng, 300)
    gz = gz_level(text, 6)
    for slice_kib in (64, 72, 80, 96):
        (got,), info = drain(ctx, [gz], slice_kib)
        assert got == text and info["n_slices"] >= 2
    # a text whose every block copies from the 32 KiB in front of it: one 20 kB piece over and over
    piece = fastq_text(rng, 80)
    text = piece * 150
    (got,), info = drain(ctx, [gz_level(text, 6)], 64)
    assert got == text


@pytest.mark.parametrize("delta", [0, -1, 1])
def test_member_boundary_on_before_and_behind_a_slice_end(ctx, delta):
    rng = np.random.default_rng(12)
    a, b = fastq_text(rng, 2600), fastq_text(rng, 2000)
    ga, gb = gz_level(a, 6), gz_level(b, 6)
    ctx.set_option("inflate_slice_bytes", str(len(ga) - delta))              # the first slice ends `delta` bytes in front of the member's end
    st = S.InflateStream(ctx, [ga + gb])
    try:
        w = st.next()
        assert w.read_file(0) == a and w.n_members == 1 and not st.finished[0]
        w2 = st.next(None, [len(a)])
        assert w2.read_file(0) == b and st.finished[0]
        w.close(); w2.close()
    finally:
        st.close()
        ctx.set_option("inflate_slice_bytes", "0")


def test_bgzf_members_small_members_stored_and_fixed_blocks(ctx):
    rng = np.random.default_rng(13)
    a, small, c = fastq_text(rng, 3000), fastq_text(rng, 5), fastq_text(rng, 2500)
    (got,), info = drain(ctx, [bgzf_compress(a)], 64)                                     # BGZF, its empty final member included
    assert got == a and info["n_slices"] >= 3
    multi = gz_level(a, 6) + gz_level(small, 6) + gz_level(b"", 6) + gz_level(c, 1)       # small and empty members go through zlib
    (got,), info = drain(ctx, [multi], 64)
    assert got == a + small + c
    noise = rng.integers(0, 256, size=100000, dtype=np.uint8).tobytes()                  # stored blocks between dynamic ones
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    mixed = co.compress(a) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(noise) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(c) + co.flush()
    (got,), info = drain(ctx, [mixed], 64)
    assert got == a + noise + c
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    part = co.compress(a) + co.flush(zlib.Z_SYNC_FLUSH)
    # fixed-Huffman blocks between dynamic ones: short pieces flushed one by one (zlib writes a short block with the fixed code)
    for i in range(40):
        part += co.compress(small[:40 + i]) + co.flush(zlib.Z_SYNC_FLUSH)
    part += co.compress(c) + co.flush()
    want = a + b"".join(small[:40 + i] for i in range(40)) + c
    assert zlib.decompress(part, 31) == want
    (got,), info = drain(ctx, [part], 64)
    assert got == want
    # a member that spans three slices and more, between two others
    (got,), info = drain(ctx, [gz_level(small, 6) + gz_level(a + c, 6) + gz_level(small, 6)], 64)
    assert got == small + a + c + small and info["n_slices"] >= 4


def test_a_first_block_larger_than_the_slice_and_one_that_never_fits(ctx):
    rng = np.random.default_rng(15)
    a, c = fastq_text(rng, 1200), fastq_text(rng, 1200)
    noise = rng.integers(0, 256, size=300000, dtype=np.uint8).tobytes()      # stored blocks: ONE chain block of 300 KB
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    gz = co.compress(a) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(noise) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(c) + co.flush()
    (got,), info = drain(ctx, [gz], 64)
    assert got == a + noise + c
    big = rng.integers(0, 256, size=(64 * KiB << 6) + (1 << 20) + 200000, dtype=np.uint8).tobytes()
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    gz = co.compress(a) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(big) + co.flush()
    with pytest.raises(SylphHipError) as ei:
        drain(ctx, [gz], 64)
    assert ei.value.code == ERR_FORMAT and "does not fit the slice" in str(ei.value)


def test_blocks_that_outgrow_their_regions_are_decoded_again(ctx, texts, gzs, monkeypatch):
    """SYLPH_HIP_INFLATE_REGION_RATIO=1: every block outgrows its region.  It first moves to one of the 96 regions of the spill arena; the
    blocks that find it empty run dry and are decoded again.  BGZF members of 4 kB of text are ~1 KB of gzip each: a slice of 128 KiB
    holds well over 96 of them."""
    monkeypatch.setenv("SYLPH_HIP_INFLATE_REGION_RATIO", "1")
    for gz, at_least in ((gzs[6], 0), (bgzf_compress(texts[6], block=4000), 20)):
        ctx.set_option("inflate_slice_bytes", str(128 * KiB))
        st = S.InflateStream(ctx, [gz])
        try:
            got, again, prev = bytearray(), 0, None
            while not st.finished[0]:
                w = st.next()
                if prev is not None:
                    prev.close()
                prev = w
                got += w.read_file(0)
                again += w.n_decoded_again
            prev.close()
            assert bytes(got) == texts[6] and again >= at_least and st.info()["n_slices"] > 1
        finally:
            st.close()
            ctx.set_option("inflate_slice_bytes", "0")


def test_damage_is_err_format_from_next_and_the_context_is_fine_afterwards(ctx, texts, gzs):
    text, gz = texts[6], gzs[6]
    st = S.InflateStream(ctx, [gz], 64 * KiB)
    ends = []                                              # text bytes after every slice of the good file
    prev = None
    while not st.finished[0]:
        w = st.next()
        if prev is not None:
            prev.close()
        prev = w
        ends.append((ends[-1] if ends else 0) + w.files[0][1])
    prev.close()
    st.close()
    assert len(ends) >= 5 and ends[-1] == len(text)
    crc = bytearray(gz); crc[-8] ^= 1
    isize = bytearray(gz); isize[-1] ^= 1
    # A flipped bit in the third slice that the slice itself can see: the text as eight members, one bit of the third member's CRC.
    # (Damage among a block's symbols need not break anything a decoder checks before the member's CRC: every bit pattern is some code
    #  of a complete Huffman code, and the codes fall back into step — zlib hands such bytes out too, and fails at the trailer.  That is
    #  the "symbols" case below: 3 kB of 0xFF in the third slice; the bytes handed out must be the ones zlib's streaming inflate gives.)
    step = len(text) // 8 + 1
    parts = [text[i:i + step] for i in range(0, len(text), step)]
    comp = [gz_level(p, 6) for p in parts]
    multi = bytearray(b"".join(comp))
    end3 = sum(len(c) for c in comp[:3])
    assert 2 * 64 * KiB < end3 - 8                                              # the third member's trailer lies behind two slices
    multi[end3 - 8] ^= 0x10
    symbols = bytearray(gz)
    symbols[(len(gz) * 5) // 16:(len(gz) * 5) // 16 + 3000] = b"\xff" * 3000

    def zlib_gives(data):
        d, out = zlib.decompressobj(31), bytearray()
        try:
            for i in range(0, len(data), 4096):
                out += d.decompress(data[i:i + 4096])
        except zlib.error:
            return bytes(out)
        return bytes(out)
    cases = {"third slice": (bytes(multi), len(parts[0]) + len(parts[1])), "symbols": (bytes(symbols), ends[0]), "crc": (bytes(crc), ends[-2]),
             "isize": (bytes(isize), ends[-2]), "truncated": (gz[:-3], ends[-2]), "cut in half": (gz[:len(gz) // 2], 1), "garbage": (gz + b"garbage", ends[-2])}
    for name, (bad, at_least) in cases.items():
        st = S.InflateStream(ctx, [bad], 64 * KiB)
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
        assert len(got) >= at_least, name
        if name == "symbols":
            z = zlib_gives(bad)
            k = min(len(z), len(got))
            assert k >= ends[0] and bytes(got[:k]) == z[:k]                      # never a byte zlib would not have produced before that point
        else:
            assert bytes(got) == text[:len(got)], name                           # what the earlier slices gave was right
        if name == "third slice":
            assert len(got) < len(parts[0]) + len(parts[1]) + len(parts[2])      # declined at the slice that holds it
        with pytest.raises(SylphHipError) as ei:                                 # the stream is dead
            st.next()
        assert ei.value.code == ERR_FORMAT
        st.close()
    # the same context inflates a good file through both roads
    t = S.Inflated(ctx, gz)
    assert t.read().tobytes() == text
    t.close()
    (got,), _ = drain(ctx, [gz], 64)
    assert got == text


def test_scratch_is_a_function_of_the_slice_not_of_the_file(ctx, texts):
    short = texts[6]
    long_ = short * 4
    _, a = drain(ctx, [gz_level(short, 6)], 128)
    (got,), b = drain(ctx, [gz_level(long_, 6)], 128)
    assert got == long_ and b["n_slices"] >= 3 * a["n_slices"]
    # per-call variance in the regions and the redo buffer is the only part that depends on the file; the whole-file road needs 4x
    assert a["peak_scratch_bytes"] > 0 and b["peak_scratch_bytes"] <= 1.5 * a["peak_scratch_bytes"]
    assert b["peak_window_bytes"] <= 2 * a["peak_window_bytes"]


def test_the_whole_file_road_declines_at_its_limit_and_the_stream_takes_the_file(ctx, texts, gzs):
    """"inflate_whole_max_bytes" lowers the whole-file road's limit (3 GiB by default) for the tests; the stream has none"""
    with pytest.raises(SylphHipError):
        ctx.set_option("inflate_whole_max_bytes", str(4 << 30))              # never above the road's own limit
    ctx.set_option("inflate_whole_max_bytes", str(len(gzs[6])))
    try:
        with pytest.raises(SylphHipError) as ei:
            S.Inflated(ctx, gzs[6])
        assert ei.value.code == ERR_FORMAT
        small = gz_level(texts[6][:100000], 6)
        t = S.Inflated(ctx, small)                                           # below the limit: as ever
        assert t.read().tobytes() == texts[6][:100000]
        t.close()
        (got,), _ = drain(ctx, [gzs[6]], 128)
        assert got == texts[6]
    finally:
        ctx.set_option("inflate_whole_max_bytes", str(3 << 30))
    t = S.Inflated(ctx, gzs[6])
    assert t.n_bytes == len(texts[6])
    t.close()
    with pytest.raises(SylphHipError):
        ctx.set_option("inflate_slice_bytes", "1000")                        # a slice is 64 KiB at least


# ---- sylph_fastq_index_window

def python_split(text):
    """(lengths of the sequence lines of the complete four-line records, where they end) by a split of the text"""
    lines = text.split(b"\n")[:-1]                         # only a line that ends in a newline counts
    n = len(lines) // 4
    consumed = sum(len(l) + 1 for l in lines[:4 * n])
    return [len(lines[4 * r + 1].rstrip(b"\r")) for r in range(n)], consumed


def test_fastq_index_window_against_a_python_split(ctx):
    rng = np.random.default_rng(21)
    text = fastq_text(rng, 300)
    starts = [0]
    for line in text.split(b"\n")[:-1]:
        starts.append(starts[-1] + len(line) + 1)
    cuts = {"mid-record": starts[30], "mid-line": starts[29] + 5, "behind a newline": starts[32], "inside the first record": starts[2] + 3,
            "before the first newline": 3, "the whole text": len(text), "without the last newline": len(text) - 1, "a long text": None}
    for name, cut in cuts.items():
        t = fastq_text(rng, 40000)[:-7] if cut is None else text[:cut]       # (10 MB: thousands of tiles)
        want_len, want_consumed = python_split(t)
        f = S.FastqText(ctx, t, final=0)
        try:
            assert f.n_records == len(want_len) and f.consumed == want_consumed, name
            assert f.lengths().tolist() == want_len, name
            assert f.n_bases == sum(want_len)
            if name == "inside the first record":
                assert f.n_records == 0 and f.consumed == 0
            for r in sorted({0, f.n_records // 2, f.n_records}):
                assert f.record_offset(r) == sum(len(l) + 1 for l in t.split(b"\n")[:4 * r]), (name, r)
        finally:
            f.close()
    f = S.FastqText(ctx, b"", final=0)                                      # zero records is not an error
    assert f.n_records == 0 and f.consumed == 0
    f.close()
    # a window borrowed from the device, at an odd address: the text of an inflated file from byte 3 on
    inf = S.Inflated(ctx, gz_level(b"xyz" + text[:starts[30] + 9], 6))
    f = S.FastqText(ctx, inf.dev_ptr + 3, MEM_DEVICE, inf.n_bytes - 3, final=0)
    assert f.n_records == 7 and f.consumed == starts[28]
    f.close(); inf.close()


def test_fastq_index_window_final_is_fastq_index(ctx):
    from .test_gpu_fastq import fastq_text as records_text
    from .helpers import random_seq
    rng = np.random.default_rng(33)
    genome = random_seq(rng, 5000)
    recs = [genome[i * 100:i * 100 + 90].copy() for i in range(40)]
    good = records_text(recs, rng)
    lines = good.split(b"\n")
    for text in (good, good[:-1], good + b"\n\r\n"):
        a, b = S.FastqText(ctx, text), S.FastqText(ctx, text, final=1)
        assert (a.n_records, a.n_bases, a.lengths().tolist()) == (b.n_records, b.n_bases, b.lengths().tolist()) and b.consumed == len(text)
        assert b.record_offset(3) == sum(len(l) + 1 for l in lines[:12])
        a.close(); b.close()
    bad = {
        "empty": b"",
        "only blank space": b"\n\n\r\n",
        "fasta": b">a\nACGT\n>b\nGGCC\n",
        "three lines": b"@a\nACGT\n+\n",
        "a record without its '@'": good.replace(b"@read7 ", b"read7 ", 1),
        "a record without its '+'": b"\n".join(lines[:10] + [b"-"] + lines[11:]),
        "quality shorter than the sequence": b"\n".join(lines[:7] + [lines[7][:-1]] + lines[8:]),
        "a blank line between records": b"\n".join(lines[:8] + [b""] + lines[8:]),
        "multi-line sequence": b"@a\nACGT\nACGT\n+\nIIIIIIII\n",
        "five lines": good + b"@x\n",
    }
    for name, text in bad.items():
        codes = []
        for final in (None, 1):
            with pytest.raises(SylphHipError) as ei:
                S.FastqText(ctx, text, final=final)
            codes.append(ei.value.code)
        assert codes == [ERR_FORMAT, ERR_FORMAT], name
    # a window refuses what it can already see: a complete record that is none
    for name in ("a record without its '@'", "a record without its '+'", "quality shorter than the sequence", "multi-line sequence"):
        with pytest.raises(SylphHipError) as ei:
            S.FastqText(ctx, bad[name], final=0)
        assert ei.value.code == ERR_FORMAT, name
    f = S.FastqText(ctx, good, final=0)                                      # ... and the context is none the worse for it
    assert f.n_records == len(recs)
    f.close()


def _window_is_python_split(ctx, t, tag):
    want_len, want_consumed = python_split(t)
    f = S.FastqText(ctx, t, final=0)
    try:
        assert f.n_records == len(want_len) and f.consumed == want_consumed, tag
        assert f.lengths().tolist() == want_len and f.n_bases == sum(want_len), tag
        for r in sorted({0, f.n_records // 2, f.n_records}):
            assert f.record_offset(r) == sum(len(l) + 1 for l in t.split(b"\n")[:4 * r]), (tag, r)
    finally:
        f.close()


def test_fastq_index_window_of_crlf_text(ctx):
    text = fastq_text(np.random.default_rng(21), 300).replace(b"\n", b"\r\n")
    starts = [0]
    for line in text.split(b"\n")[:-1]:
        starts.append(starts[-1] + len(line) + 1)
    assert len(starts) == 1201 and python_split(text) == (python_split(text.replace(b"\r", b""))[0], len(text))
    for name, cut in {"mid-record": starts[30], "mid-line": starts[29] + 5, "behind a newline": starts[32], "between '\\r' and '\\n'": starts[33] - 1}.items():
        _window_is_python_split(ctx, text[:cut], name)


def test_fastq_index_window_is_not_trimmed(ctx):
    text = fastq_text(np.random.default_rng(21), 300)
    for tail in (b"\n", b"\n\n\n"):                        # blank lines are lines: fewer than four of them are no record yet
        f = S.FastqText(ctx, text + tail, final=0)
        assert f.n_records == 300 and f.consumed == len(text), tail
        assert f.record_offset(300) == len(text)
        f.close()
    with pytest.raises(SylphHipError) as ei:               # four of them are a complete record that is none
        S.FastqText(ctx, text + b"\n\n\n\n", final=0)
    assert ei.value.code == ERR_FORMAT
    for tail in (b"\n", b"\n\n\n", b"\n\n\n\n"):           # the end of the text: trailing blank space is trimmed, as sylph_fastq_index does
        f = S.FastqText(ctx, text + tail, final=1)
        assert f.n_records == 300 and f.consumed == len(text + tail), tail
        f.close()


def test_a_window_index_pushes_like_a_whole_one(ctx):
    from .test_gpu_parity import assert_same_sketch
    text, mate2 = fastq_text(np.random.default_rng(21), 300), fastq_text(np.random.default_rng(22), 300)

    def sketch(*fs):
        sk = S.ReadSketcher(ctx, c=5, paired=len(fs) == 2)
        try:
            sk.push_fastq(*fs)
            return sk.finish()
        finally:
            sk.close()
    idx = {final: S.FastqText(ctx, text, final=final) for final in (None, 1, 0)}
    whole2 = S.FastqText(ctx, mate2)
    try:
        assert [f.n_records for f in idx.values()] == [300, 300, 300] and idx[0].consumed == len(text)
        want = sketch(idx[None])
        assert len(want["kmers"]) > 1000
        for final in (1, 0):
            assert_same_sketch(sketch(idx[final]), want, final)
        assert_same_sketch(sketch(idx[0], whole2), sketch(idx[None], whole2), "pair: mate 1 from a window")
    finally:
        for f in list(idx.values()) + [whole2]:
            f.close()
