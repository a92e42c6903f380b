"""The scaffold the two device streams share (csrc/decode_host.h StreamBase, stream_open_args, stream_next_entry, stream_info,
stream_destroy, kept_tails; behind sylph_inflate_stream_* and sylph_bunzip2_stream_*): the argument checks and their messages, a
declined call's error, what it leaves of the stream and what it gives back, two files in one stream — for gzip and bzip2 alike.  Every
file is a FASTQ text of a few records: one slice."""
import bz2
import ctypes as C
import zlib

import numpy as np
import pytest

import sylph_amd as S
from sylph_amd.binding import ERR_FORMAT, MEM_DEVICE, MEM_HOST, SylphHipError, load

pytestmark = pytest.mark.gpu

ERR_INVALID = -1


def gz(data):
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    return co.compress(data) + co.flush()


DECODERS = {
    "gzip": dict(whole=S.Inflated, stream=S.InflateStream, name="sylph_inflate_stream", pack=gz),
    "bzip2": dict(whole=S.Bunzipped, stream=S.Bunzip2Stream, name="sylph_bunzip2_stream", pack=lambda d: bz2.compress(d, 9)),
}


@pytest.fixture(params=sorted(DECODERS))
def dec(request):
    return DECODERS[request.param]


def fastq_text(seed, n_records):
    rng = np.random.default_rng(seed)
    return b"".join(b"@r%d\n" % i + rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=60).tobytes() + b"\n+\n" + b"F" * 60 + b"\n" for i in range(n_records))


def last_error():
    return load().sylph_last_error().decode("utf-8", "replace")


def raw_open(dec, ctx, files, n_files=None, mem=MEM_HOST, ptrs=True, out=True):
    """<name>_open itself; files: bytes, or None for a null pointer -> (return code, last error, the handle it left in *out)"""
    keeps = [None if f is None else np.frombuffer(f, dtype=np.uint8) for f in files]
    p = (C.c_void_p * len(files))(*[None if k is None else k.ctypes.data for k in keeps])
    n = (C.c_uint64 * len(files))(*[5 if f is None else len(f) for f in files])
    h = C.c_void_p(0xDEAD)
    rc = getattr(load(), dec["name"] + "_open")(ctx._h, p if ptrs else None, n, len(files) if n_files is None else n_files, mem, 0, C.byref(h) if out else None)
    err = last_error()
    if rc == 0:
        getattr(load(), dec["name"] + "_destroy")(h)
    return rc, err, h.value


def raw_next(dec, st, keep_from=None, window=True):
    """<name>_next itself on the handle st (a c_void_p or None) -> (return code, last error); a window it hands out is closed"""
    keep = (C.c_uint64 * len(keep_from))(*keep_from) if keep_from is not None else None
    w = C.c_void_p()
    rc = getattr(load(), dec["name"] + "_next")(st, None, keep, C.byref(w) if window else None, None)
    err = last_error()
    if rc == 0:
        load().sylph_inflated_destroy(w)
    return rc, err


def test_open_with_bad_arguments_is_invalid(ctx, dec):
    good = dec["pack"](fastq_text(1, 3))
    assert raw_open(dec, ctx, [good], ptrs=False)[:2] == (ERR_INVALID, "null argument")
    assert raw_open(dec, ctx, [good], out=False)[:2] == (ERR_INVALID, "null argument")
    assert raw_open(dec, ctx, [good, None])[:2] == (ERR_INVALID, "null argument")
    assert raw_open(dec, ctx, [good], n_files=0)[:2] == (ERR_INVALID, "null argument")
    assert raw_open(dec, ctx, [good], mem=MEM_DEVICE)[:2] == (ERR_INVALID, f"{dec['name']}_open: the compressed bytes must lie in host memory (mem kind {MEM_DEVICE})")
    assert raw_open(dec, ctx, [good])[0] == 0


def test_open_declines_another_format(ctx, dec):
    other = DECODERS["bzip2" if dec["name"] == "sylph_inflate_stream" else "gzip"]["pack"](fastq_text(2, 3))
    good = dec["pack"](fastq_text(2, 3))
    for files in ([other], [good, other], [fastq_text(2, 3)]):
        rc, err, h = raw_open(dec, ctx, files)
        assert rc == ERR_FORMAT and err.startswith(f"{dec['name']}_open: declined:"), err
        assert h is None                                  # *out was set to null


def test_next_with_bad_arguments_is_invalid(ctx, dec):
    s = dec["stream"](ctx, [dec["pack"](fastq_text(3, 3))])
    try:
        assert raw_next(dec, None) == (ERR_INVALID, "null argument")
        assert raw_next(dec, s._h, window=False) == (ERR_INVALID, "null argument")
        w = s.next()                                      # neither call gave the stream up
        assert w.read_file(0) == fastq_text(3, 3)
        w.close()
    finally:
        s.close()


def test_two_files_in_one_stream(ctx, dec):
    a, b = fastq_text(4, 4), fastq_text(5, 3)
    assert 300 < len(b) < len(a) < 1000
    s = dec["stream"](ctx, [dec["pack"](a), dec["pack"](b)])
    try:
        w = s.next()
        assert bytes(w.read()) == a + b and w.n_bytes == len(a) + len(b)
        assert w.files[0] == (w.dev_ptr, len(a)) and w.files[1] == (w.dev_ptr + len(a), len(b))          # the files' ranges tile the window
        assert s.finished == [True, True]
        w2 = s.next(keep_from=[len(a), len(b)])
        assert w2.n_bytes == 0 and [n for _, n in w2.files] == [0, 0] and s.finished == [True, True]
        w2.close()
        w.close()
        info = s.info()
        assert info["n_slices"] == 2 and info["text_bytes"] == len(a) + len(b)
    finally:
        s.close()


def test_keep_from_beyond_the_previous_window(ctx, dec):
    a = fastq_text(6, 4)
    s = dec["stream"](ctx, [dec["pack"](a)])
    try:
        w = s.next()
        assert w.read_file(0) == a
        rc, err = raw_next(dec, s._h, keep_from=[len(a) + 1])
        assert rc == ERR_INVALID and err == f"{dec['name']}_next: keep_from[0] = {len(a) + 1} lies behind the previous window ({len(a)} bytes)", err
        # a call that failed, for whatever reason, gives the stream up
        assert raw_next(dec, s._h, keep_from=[0]) == (ERR_FORMAT, f"{dec['name']}_next: the stream was given up by an earlier call")
        assert s.info()["n_slices"] == 1 and s.info()["text_bytes"] == len(a)
        w.close()
    finally:
        s.close()


def test_damage_is_declined_by_next_and_the_stream_is_given_up(ctx, dec):
    text = fastq_text(7, 4)
    packed = dec["pack"](text)
    s = dec["stream"](ctx, [packed[:len(packed) // 2]])
    try:
        rc, err = raw_next(dec, s._h)
        assert rc == ERR_FORMAT and err.startswith(f"{dec['name']}_next: declined:"), err
        assert raw_next(dec, s._h) == (ERR_FORMAT, f"{dec['name']}_next: the stream was given up by an earlier call")
    finally:
        s.close()
    assert s._h is None
    # the same context decodes a good file through both roads
    t = dec["whole"](ctx, [packed])
    assert bytes(t.read()) == text
    t.close()
    s = dec["stream"](ctx, [packed])
    try:
        w = s.next()
        assert w.read_file(0) == text and s.finished == [True]
        w.close()
    finally:
        s.close()


def test_a_stream_destroyed_after_a_declined_next_gives_its_context_reference_back(dec):
    packed = dec["pack"](fastq_text(8, 4))
    own = S.Context(0)
    try:
        s = dec["stream"](own, [packed[:len(packed) // 2]])
        with pytest.raises(SylphHipError) as e:
            s.next()
        assert e.value.code == ERR_FORMAT
        s.close()
    finally:
        own.close()
    assert not own._h
