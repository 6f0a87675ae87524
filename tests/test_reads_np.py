"""The numpy reference of the read-editing calls (tests/reads_np.py) against plain Python: reads as a list of `bytes`, clips as
slices.  Python's slice s[a:b] clips to the string by itself, which is the span rule of kmx.h said another way; the cases below name
every branch of that rule in both modes.  No GPU."""
import numpy as np
import pytest

from tests import reads_np
from tests.reads_np import span_word


def _batch(reads, first=0):
    """list of bytes -> (bases with `first` bytes of padding in front, offsets starting at `first`)"""
    bases = np.frombuffer(b"." * first + b"".join(reads), np.uint8)
    offsets = (np.cumsum([0] + [len(r) for r in reads]) + first).astype(np.uint64)
    return bases, offsets


def _cat(parts):
    return np.frombuffer(b"".join(parts), np.uint8), np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)


def _clip_py(read, start, length, span_k):
    """the span rule with slices: length counts bases (span_k == 0) or windows of span_k bases"""
    if span_k > 0:
        length = 0 if length == 0 else length + span_k - 1
    return read[start:start + length]


READS = [b"ACGTACGTAC", b"", b"TTTT", b"G", b"", b"", b"CCCCCCCCCCCCCCCCCCCCCCCCC", b"AG"]

# (start, length) per read of READS: whole, empty, past the end, start == L, start > L, zero length, 32-bit extremes
SPANS = [
    [(0, 10), (0, 0), (1, 2), (0, 1), (0, 5), (3, 3), (5, 100), (2, 1)],
    [(3, 4), (0, 7), (4, 1), (1, 1), (0, 0), (0, 1), (24, 1), (1, 0xFFFFFFFF)],
    [(9, 1), (1, 1), (0, 0xFFFFFFFF), (0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0, 0), (25, 1), (0xFFFFFFFF, 1)],
    [(10, 1), (0, 0), (3, 1), (0, 2), (0, 0), (0, 0), (0, 25), (0, 2)],
]


@pytest.mark.parametrize("span_k", (0, 1, 3, 31))
@pytest.mark.parametrize("first", (0, 5))
@pytest.mark.parametrize("case", range(len(SPANS)))
def test_select_is_slicing(case, first, span_k):
    bases, offsets = _batch(READS, first)
    span = np.array([span_word(s, n) for s, n in SPANS[case]], np.uint64)
    want = [_clip_py(r, s, n, span_k) for r, (s, n) in zip(READS, SPANS[case])]
    out, off, idx = reads_np.select_np(bases, len(READS), 0, offsets, span=span, span_k=span_k)
    wb, wo = _cat(want)
    assert np.array_equal(out, wb) and np.array_equal(off, wo) and np.array_equal(idx, np.arange(len(READS)))
    # min_len on the boundary: a clip of exactly min_len stays, one shorter goes
    for min_len in (1, 2, 4, 25, 26):
        out, off, idx = reads_np.select_np(bases, len(READS), 0, offsets, span=span, span_k=span_k, min_len=min_len)
        kept = [i for i, w in enumerate(want) if len(w) >= min_len]
        wb, wo = _cat([want[i] for i in kept])
        assert np.array_equal(out, wb) and np.array_equal(off, wo) and idx.tolist() == kept


def test_window_span_rule_named_cases():
    """span_k > 0: len == 0 keeps nothing; len windows cover len + span_k - 1 bases; clipped to the read"""
    bases, offsets = _batch([b"ACGTACGTAC"])
    for (start, length, k), want in {(0, 0, 4): b"", (0, 1, 4): b"ACGT", (2, 3, 4): b"GTACGT", (6, 1, 4): b"GTAC", (7, 1, 4): b"TAC",
                                     (9, 5, 4): b"C", (10, 1, 4): b"", (0, 7, 4): b"ACGTACGTAC", (0, 8, 4): b"ACGTACGTAC"}.items():
        out, off, _ = reads_np.select_np(bases, 1, 0, offsets, span=np.array([span_word(start, length)]), span_k=k)
        assert bytes(out) == want and off.tolist() == [0, len(want)], (start, length, k)


def test_select_keep_and_empty_reads():
    bases, offsets = _batch(READS, 3)
    keep = np.array([1, 1, 0, 7, 0, 1, 1, 0], np.uint8)
    out, off, idx = reads_np.select_np(bases, len(READS), 0, offsets, keep=keep)
    kept = [i for i in range(len(READS)) if keep[i]]
    wb, wo = _cat([READS[i] for i in kept])
    assert np.array_equal(out, wb) and np.array_equal(off, wo) and idx.tolist() == kept   # min_len == 0 keeps the empty reads 1 and 5
    out, off, idx = reads_np.select_np(bases, len(READS), 0, offsets, keep=np.zeros(8, np.uint8))
    assert len(out) == 0 and off.tolist() == [0] and len(idx) == 0
    out, off, idx = reads_np.select_np(bases, 0, 0, offsets[:1])
    assert len(out) == 0 and off.tolist() == [0] and len(idx) == 0


def test_uniform_reads_and_long_reads():
    rng = np.random.default_rng(5)
    bases = rng.choice(np.frombuffer(b"ACGT", np.uint8), 7 * 13).astype(np.uint8)
    reads = [bytes(bases[i * 13:(i + 1) * 13]) for i in range(7)]
    span = np.array([span_word(i, 2 * i) for i in range(7)], np.uint64)
    out, off, idx = reads_np.select_np(bases, 7, 13, None, span=span, min_len=1)
    want = [r[i:3 * i] for i, r in enumerate(reads)]
    wb, wo = _cat([w for w in want if w])
    assert np.array_equal(out, wb) and np.array_equal(off, wo) and idx.tolist() == [i for i, w in enumerate(want) if w]
    # a read of 2^31 bases or more counts as empty (only its offsets are looked at)
    a, L = reads_np.read_bounds(3, 0, np.array([0, 5, 5 + 2**31, 9 + 2**31], np.uint64))
    assert L.tolist() == [5, 0, 4] and a.tolist() == [0, 5, 5 + 2**31]
    a, L = reads_np.read_bounds(2, 2**31, None)
    assert L.tolist() == [0, 0]


def test_gather_is_indexing():
    bases, offsets = _batch(READS, 2)
    span = np.array([span_word(1, 3)] * len(READS), np.uint64)
    for index in ([7, 6, 5, 4, 3, 2, 1, 0], [0, 0, 6, 6, 6, 3], [8, 0, 2**40, 3, 2**64 - 1], []):
        out, off = reads_np.gather_np(bases, len(READS), 0, np.array(index, np.uint64), offsets)
        wb, wo = _cat([READS[i] if i < len(READS) else b"" for i in index])
        assert np.array_equal(out, wb) and np.array_equal(off, wo)
        out, off = reads_np.gather_np(bases, len(READS), 0, np.array(index, np.uint64), offsets, span=span)   # the span of the SOURCE read
        wb, wo = _cat([READS[i][1:4] if i < len(READS) else b"" for i in index])
        assert np.array_equal(out, wb) and np.array_equal(off, wo)
    out, off = reads_np.gather_np(bases, len(READS), 0, np.arange(len(READS), dtype=np.uint64), offsets)
    sel = reads_np.select_np(bases, len(READS), 0, offsets)
    assert np.array_equal(out, sel[0]) and np.array_equal(off, sel[1])


def test_partition_is_a_stable_sort():
    bases, offsets = _batch(READS)
    labels = [5, -1, 2, 5, 2, -7, 900, 2]
    out, off, index, distinct, group_offsets = reads_np.partition_np(bases, len(READS), 0, labels, offsets)
    order = [i for lab in sorted(set(v for v in labels if v >= 0)) for i in range(len(READS)) if labels[i] == lab]
    assert index.tolist() == order == [2, 4, 7, 0, 3, 6]
    assert distinct.tolist() == [2, 5, 900] and group_offsets.tolist() == [0, 3, 5, 6]
    wb, wo = _cat([READS[i] for i in order])
    assert np.array_equal(out, wb) and np.array_equal(off, wo)
    out, off, index, distinct, group_offsets = reads_np.partition_np(bases, len(READS), 0, [-1] * 8, offsets)
    assert len(out) == 0 and off.tolist() == [0] and len(distinct) == 0 and group_offsets.tolist() == [0]
