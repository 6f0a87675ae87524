"""Pins the host references of tests/fastx_out_np.py (CPU only): an image that format_np lays out, parsed back by the oracle's
fastx_parse, by tests/quality_np.fastq_quals and by fastq_names, is the batch it was made from; fastq_names against a line walk
written another way on every FASTQ text of tests/fastx_cases.EDGE_TEXTS; generated decimal names at the edges of u64; the record
lengths kmx.h states."""
import numpy as np
import pytest

from tests import fastx_out_np as F
from tests import quality_np as Q
from tests.fastx_cases import EDGE_TEXTS, fastq_text
from tests.reads_dev import ragged

FASTQ, FASTA = F.FASTQ, F.FASTA
L0 = 37


def _batch(rng, lens):
    reads = [bytes(rng.choice(list(b"ACGTacgtN"), n).astype(np.uint8)) for n in lens]
    quals = [bytes(rng.choice(list(b"@>+IIFF#5"), n).astype(np.uint8)) for n in lens]
    names = [b"@r%d/%d x" % (i, n) if i % 5 else b"@" for i, n in enumerate(lens)]
    return reads, quals, names


@pytest.mark.parametrize("width", [0, 1, 7, 60, L0, L0 - 1, L0 + 1])
def test_fasta_parses_back(orc, width):
    rng = np.random.default_rng(7 + width)
    lens = [L0, 0, 1, L0 - 1, L0 + 1, 2 * L0, 0, 60, 61, 119, 120, 121, 7, 14] + list(rng.integers(0, 200, 30))
    reads, _, names = _batch(rng, lens)
    bases, off = ragged(reads)
    nm, noff = ragged(names)
    img, rec = F.format_np(bases, len(lens), 0, off, names=nm, name_offsets=noff, fmt=FASTA, line_width=width)
    text = img.tobytes()
    assert [len(x) for x in F.records_np(bases, len(lens), 0, off, names=nm, name_offsets=noff, fmt=FASTA, line_width=width)] == \
        [F.record_len(n, len(names[i]) - 1, FASTA, width) for i, n in enumerate(lens)]
    assert int(rec[-1]) == len(text) and all(text[int(o):int(o) + 1] == b">" for o in rec[:-1])
    if width:
        assert max(len(ln) for ln in text.split(b"\n") if ln[:1] != b">") <= width
    got_b, got_o = orc.fastx_parse(text, FASTA)
    assert np.array_equal(got_b, bases) and np.array_equal(np.asarray(got_o, np.uint64), off)
    headers = [ln for ln in text.split(b"\n") if ln[:1] == b">"]
    assert headers == [b">" + n[1:] for n in names]


@pytest.mark.parametrize("fill", [False, True])
def test_fastq_parses_back(orc, fill):
    rng = np.random.default_rng(11 + fill)
    lens = [L0, 0, 1, 0, 0, 150] + list(rng.integers(0, 200, 40))
    reads, quals, names = _batch(rng, lens)
    bases, off = ragged(reads, first=5)
    ql, _ = ragged(quals, first=5)
    nm, noff = ragged(names, first=3)
    img, rec = F.format_np(bases, len(lens), 0, off, quals=None if fill else ql, names=nm, name_offsets=noff, fmt=FASTQ, qual_fill=ord("#"))
    text = img.tobytes()
    assert np.array_equal(np.diff(rec.astype(np.int64)), [F.record_len(n, len(names[i]) - 1, FASTQ) for i, n in enumerate(lens)])
    got_b, got_o = orc.fastx_parse(text, FASTQ)
    assert got_b.tobytes() == b"".join(reads) and np.array_equal(np.asarray(got_o, np.uint64), off - np.uint64(5))
    got_q, got_qo = Q.fastq_quals(text)
    assert got_q.tobytes() == (b"".join(b"#" * n for n in lens) if fill else b"".join(quals)) and np.array_equal(got_qo, off - np.uint64(5))
    got_n, got_no = F.fastq_names(text)
    assert got_n.tobytes() == b"".join(names) and np.array_equal(got_no, noff - np.uint64(3))


def test_uniform_reads_and_name_skip():
    bases = np.frombuffer(b"ACGTTGCAGG", np.uint8)
    nm, noff = ragged([b"@ab", b"x"])
    assert F.format_np(bases, 2, 5, names=nm, name_offsets=noff, name_skip=0, fmt=FASTA)[0].tobytes() == b">@ab\nACGTT\n>x\nGCAGG\n"
    assert F.format_np(bases, 2, 5, names=nm, name_offsets=noff, name_skip=2, fmt=FASTA, line_width=2)[0].tobytes() == b">b\nAC\nGT\nT\n>\nGC\nAG\nG\n"
    assert F.format_np(bases, 2, 5, name_base=9, qual_fill=ord("!"))[0].tobytes() == b"@9\nACGTT\n+\n!!!!!\n@10\nGCAGG\n+\n!!!!!\n"
    # an offsets pair that descends is an empty read; an empty read has one empty sequence line
    off = np.array([4, 2, 6], np.uint64)
    assert F.format_np(bases, 2, 0, off, fmt=FASTA, line_width=3)[0].tobytes() == b">0\n\n>1\nGTT\nG\n"
    assert F.format_np(bases, 2, 0, off, fmt=FASTQ)[0].tobytes() == b"@0\n\n+\n\n@1\nGTTG\n+\nIIII\n"
    with pytest.raises(ValueError):
        F.format_np(bases, 2, 5, fmt=FASTQ, line_width=4)
    with pytest.raises(ValueError):
        F.format_np(bases, 2, 5, fmt=0)


@pytest.mark.parametrize("base, want", [(0, b"0"), (9, b"9"), (10, b"10"), (2**64 - 1, b"18446744073709551615"), (2**64, b"0")])
def test_decimal_names(base, want):
    assert F.decimal_name(base, 0) == want
    assert F.decimal_name(2**64 - 1, 1) == b"0" and F.decimal_name(2**64 - 2, 3) == b"1" and F.decimal_name(99, 1) == b"100"
    img, rec = F.format_np(np.zeros(0, np.uint8), 2, 0, name_base=2**64 - 1, fmt=FASTA)
    assert img.tobytes() == b">18446744073709551615\n\n>0\n\n" and rec.tolist() == [0, 23, 27]


def _names_by_walk(text):
    """the names by a walk over the bytes: a line counter, no split"""
    names, cur, line = [], bytearray(), 0
    open_line = False
    for c in text:
        if c == 10:
            if line % 4 == 0:
                names.append(bytes(cur))
            cur, line, open_line = bytearray(), line + 1, False
            continue
        open_line = True
        if line % 4 == 0 and c != 13:
            cur.append(c)
    if open_line and line % 4 == 0:
        names.append(bytes(cur))
    return names


@pytest.mark.parametrize("i", [i for i, t in enumerate(EDGE_TEXTS) if t[:1] == b"@" or not t])
def test_fastq_names_on_edge_texts(i):
    text = EDGE_TEXTS[i]
    names, off = F.fastq_names(text)
    want = _names_by_walk(text)
    assert names.tobytes() == b"".join(want) and off.tolist() == np.concatenate([[0], np.cumsum([len(n) for n in want])]).astype(np.uint64).tolist()
    # one name per quality line, or one more where the text ends inside a record
    nq = len(Q.fastq_quals(text)[1]) - 1
    assert len(want) - nq in (0, 1)


def test_fastq_names_counts_and_crlf():
    rng = np.random.default_rng(3)
    for crlf in (False, True):
        for trail in (False, True):
            text = fastq_text(rng, 20, 0, 30, crlf=crlf, trail=trail)
            names, off = F.fastq_names(text)
            assert len(off) == 21 and names.tobytes() == b"".join(_names_by_walk(text)) and b"\r" not in names.tobytes()
    assert len(F.fastq_names(b"@a\nAC\n+\nII\n")[1]) - 1 == 1          # the newline that ends the last quality line opens no record
    assert len(F.fastq_names(b"@a\nAC\n+\nII\n@")[1]) - 1 == 2
    assert len(F.fastq_names(b"@a\nAC\n+\nII\n\n")[1]) - 1 == 2        # an empty header line is a line
    assert F.fastq_names(b"@a\nAC\n+\nII\n\n")[0].tobytes() == b"@a"
    with pytest.raises(ValueError):
        F.fastq_names(b">a\nAC\n")
