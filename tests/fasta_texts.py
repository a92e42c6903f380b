"""FASTA texts for tests/test_fasta_plan.py and tests/test_gpu_fasta.py: records written out with a chosen line width, line end, last
newline, trailing blank lines and blank lines inside sequences; the refusal cases of sylph_fasta_index; and the records of a text as
oracle.read_fastx finds them."""
import os

import numpy as np

from oracle import oracle as O


def fasta_text(recs, ids, width=60, eol=b"\n", last_eol=True, trailing=0, blank_every=0):
    """recs: list of bytes (sequences), ids: list of bytes.  width = bases per line, or 0 for one line per record.  blank_every = k > 0: an
    empty line behind every k-th sequence line.  trailing = number of blank lines behind the last line."""
    out, n_line = [], 0
    for name, seq in zip(ids, recs):
        out.append(b">" + name + eol)
        step = width if width else max(1, len(seq))
        for i in range(0, len(seq), step):
            out.append(seq[i:i + step] + eol)
            n_line += 1
            if blank_every and n_line % blank_every == 0:
                out.append(eol)
    t = b"".join(out)
    if trailing:
        return t + eol * trailing
    if not last_eol and t.endswith(eol):
        t = t[:-len(eol)]
    return t


def random_records(rng, n_rec, max_len=400, empty_frac=0.15):
    """sequences (upper and lower case, N among them) and ids (with '>' and '@' inside) of n_rec records; some are empty, some one base"""
    alphabet = np.frombuffer(b"ACGTacgtNn", dtype=np.uint8)
    recs, ids = [], []
    for i in range(n_rec):
        u = rng.random()
        n = 0 if u < empty_frac else 1 if u < empty_frac + 0.05 else int(rng.integers(2, max_len + 1))
        recs.append(bytes(rng.choice(alphabet, size=n, p=[0.22] * 4 + [0.02] * 4 + [0.03, 0.01]).astype(np.uint8)))
        ids.append([b"contig_%d" % i, b"c%d len=%d >odd @name" % (i, n), b"", b"@%d" % i, b">%d" % i][int(rng.integers(0, 5))])
    return recs, ids


# what sylph_fasta_index refuses (SYLPH_ERR_FORMAT) besides a text of 2^32 - 4096 bytes or more and one of 2^32 lines or more
REFUSED = {
    "empty": b"",
    "fastq": b"@r1\nACGT\n+\nIIII\n",
    "a leading blank line": b"\n>a\nACGT\n",
    "a leading CRLF": b"\r\n>a\nACGT\n",
    "a leading space": b" >a\nACGT\n",
    "no '>' at all": b"ACGT\nACGT\n",
    "CR CR LF": b">a\nACGT\r\r\nGG\n",
    "CR inside a sequence line": b">a\nAC\rGT\nGG\n",
    "CR inside a header": b">a\rb\nACGT\n",
    "CR at the start of a line": b">a\n\rACGT\n",
    "CR CR at the end": b">a\nACGT\r\r",
    "old Mac line ends": b">a\rACGT\rGGCC\r",
    "CR in front of the last base": b">a\n" + b"ACGT" * 1500 + b"\rA",
}


def records_by_the_host_reader(text, tmp_path, name="t.fa"):
    """[(id, sequence)] as oracle.read_fastx reads the bytes from a file"""
    p = os.path.join(str(tmp_path), name)
    with open(p, "wb") as f:
        f.write(text)
    return O.read_fastx(p)
