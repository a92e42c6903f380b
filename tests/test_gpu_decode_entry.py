"""The entry the two device decompressors share (csrc/decode_host.h decode_entry, behind sylph_inflate_files and sylph_bunzip2_files):
the argument checks and their messages, a declined call's error and what it gives back, two files in one call — for gzip and bzip2
alike, and the one rule on which they differ (a file of no bytes may come with a null pointer to bzip2 only)."""
import bz2
import ctypes as C
import gzip
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
    "gzip": dict(cls=S.Inflated, entry="sylph_inflate_files", name="sylph_inflate", pack=gz, unpack=gzip.decompress),
    "bzip2": dict(cls=S.Bunzipped, entry="sylph_bunzip2_files", name="sylph_bunzip2", pack=lambda d: bz2.compress(d, 9), unpack=bz2.decompress),
}


@pytest.fixture(params=sorted(DECODERS))
def dec(request):
    return DECODERS[request.param]


def fastq_text(seed, n_records):
    rng = np.random.default_rng(seed)
    return b"".join(b"@r%d\n" % i + rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=60).tobytes() + b"\n+\n" + b"F" * 60 + b"\n" for i in range(n_records))


def raw_call(dec, ctx, files, n_files=None, mem=MEM_HOST, ptrs=True, out=True):
    """the C entry itself; files: bytes, or an int n for a null pointer said to hold n bytes -> (return code, last error)"""
    keeps = [None if isinstance(f, int) else np.frombuffer(f, dtype=np.uint8) for f in files]
    p = (C.c_void_p * len(files))(*[None if k is None else k.ctypes.data for k in keeps])
    n = (C.c_uint64 * len(files))(*[f if isinstance(f, int) else len(f) for f in files])
    h = C.c_void_p()
    rc = getattr(load(), dec["entry"])(ctx._h, p if ptrs else None, n, len(files) if n_files is None else n_files, mem, C.byref(h) if out else None)
    err = load().sylph_last_error().decode("utf-8", "replace")
    if rc == 0:
        load().sylph_inflated_destroy(h)
    return rc, err


def test_two_files_in_one_call(ctx, dec):
    a, b = fastq_text(1, 4), fastq_text(2, 3)
    assert 300 < len(b) < len(a) < 1000
    packed = [dec["pack"](a), dec["pack"](b) + (gz(b"") if dec["name"] == "sylph_inflate" else b"")]      # gzip's second file ends in an empty member
    assert [dec["unpack"](p) for p in packed] == [a, b]
    t = dec["cls"](ctx, packed)
    try:
        whole = bytes(t.read())
        assert whole == a + b and t.n_bytes == len(a) + len(b)
        assert t.files[0] == (t.dev_ptr, len(a)) and t.files[1] == (t.dev_ptr + len(a), len(b))          # the files' ranges tile the text
        assert bytes(t.read(0, len(a))) == a and bytes(t.read(len(a), len(b))) == b
    finally:
        t.close()


def test_bad_arguments_are_invalid(ctx, dec):
    good = dec["pack"](fastq_text(3, 3))
    assert raw_call(dec, ctx, [good], ptrs=False) == (ERR_INVALID, "null argument")
    assert raw_call(dec, ctx, [good], out=False) == (ERR_INVALID, "null argument")
    assert raw_call(dec, ctx, [good, 5]) == (ERR_INVALID, "null argument")
    assert raw_call(dec, ctx, [5]) == (ERR_INVALID, "null argument")
    assert raw_call(dec, ctx, [good], n_files=0) == (ERR_INVALID, "null argument")
    assert raw_call(dec, ctx, [good], mem=MEM_DEVICE) == (ERR_INVALID, f"{dec['name']}: the compressed bytes must lie in host memory (mem kind {MEM_DEVICE})")
    assert raw_call(dec, ctx, [good])[0] == 0


def test_a_first_file_of_another_format_is_declined(ctx, dec):
    other = DECODERS["bzip2" if dec["name"] == "sylph_inflate" else "gzip"]["pack"](fastq_text(4, 3))
    good = dec["pack"](fastq_text(4, 3))
    for files in ([other], [other, good], [fastq_text(4, 3)]):
        rc, err = raw_call(dec, ctx, files)
        assert rc == ERR_FORMAT and err.startswith(f"{dec['name']}: declined:"), err


def test_a_declined_call_gives_its_context_reference_back(dec):
    own = S.Context(0)
    try:
        text = fastq_text(5, 4)
        with pytest.raises(SylphHipError) as e:
            dec["cls"](own, [b"neither gzip nor bzip2, but long enough to hold a header"])
        assert e.value.code == ERR_FORMAT
        t = dec["cls"](own, [dec["pack"](text)])
        assert bytes(t.read()) == text
        t.close()
    finally:
        own.close()
    assert not own._h


def test_a_file_of_no_bytes_with_a_null_pointer(ctx, dec):
    good = dec["pack"](fastq_text(6, 3))
    for files in ([good, 0], [0]):
        rc, err = raw_call(dec, ctx, files)
        if dec["name"] == "sylph_bunzip2":        # the arguments pass; no bytes are no bzip2 file
            assert rc == ERR_FORMAT and err.startswith("sylph_bunzip2: declined:") and "is empty" in err, err
        else:
            assert (rc, err) == (ERR_INVALID, "null argument")
    assert raw_call(dec, ctx, [good])[0] == 0
