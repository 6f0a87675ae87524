"""Host reference of kmx_reads_select, kmx_reads_gather and Context.reads_partition (include/kmx.h, "a new batch of reads from an
old one"), in numpy: what tests/test_gpu_reads_edit.py compares the device's bytes, offsets and index words with.  Pinned against
plain Python slicing of a list of `bytes` in tests/test_reads_np.py.

A batch is (bases uint8[...], offsets uint64[n + 1]) or, for uniform reads, (bases, None) with read_len.  Span words are uint64:
start in the low 32 bits, length in the high 32."""
import numpy as np

MASK32 = np.uint64(0xFFFFFFFF)


def span_word(start, length):
    return np.uint64(int(start) | (int(length) << 32))


def read_bounds(n_reads, read_len, offsets):
    """(first byte, length) of every source read, int64; a read of 2^31 bases or more, or descending offsets: length 0"""
    if offsets is None:
        a = np.arange(n_reads, dtype=np.int64) * int(read_len)
        L = np.full(n_reads, int(read_len), np.int64)
    else:
        o = np.asarray(offsets).astype(np.int64)
        a, L = o[:n_reads], o[1:n_reads + 1] - o[:n_reads]
        L = np.where(L < 0, 0, L)
    return a, np.where(L >= 2**31, 0, L)


def clips(n_reads, read_len, offsets, span=None, span_k=0):
    """(first byte, length) of every source read's clip: the span rule of kmx.h, in Python integers per read"""
    a, L = read_bounds(n_reads, read_len, offsets)
    if span is None:
        return a, L
    src, ln = np.zeros(n_reads, np.int64), np.zeros(n_reads, np.int64)
    for r in range(n_reads):
        w = int(span[r])
        start, length = w & 0xFFFFFFFF, w >> 32
        if span_k > 0 and length > 0:
            length += span_k - 1
        if start >= int(L[r]):
            start, length = 0, 0
        else:
            length = min(length, int(L[r]) - start)
        src[r], ln[r] = int(a[r]) + start, length
    return src, ln


def _emit(bases, src, ln):
    """the clips back to back -> (bytes, offsets uint64)"""
    offsets = np.zeros(len(src) + 1, np.uint64)
    offsets[1:] = np.cumsum(ln).astype(np.uint64)
    parts = [bases[s:s + n] for s, n in zip(src.tolist(), ln.tolist()) if n]
    out = np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, np.uint8)
    return out, offsets


def select_np(bases, n_reads, read_len, offsets=None, keep=None, span=None, span_k=0, min_len=0):
    """-> (out bases, out offsets uint64[n_out + 1], index uint64[n_out])"""
    src, ln = clips(n_reads, read_len, offsets, span, span_k)
    kept = ln >= int(min_len)
    if keep is not None:
        kept &= np.asarray(keep)[:n_reads] != 0
    idx = np.nonzero(kept)[0]
    out, off = _emit(np.asarray(bases), src[idx], ln[idx])
    return out, off, idx.astype(np.uint64)


def gather_np(bases, n_reads, read_len, index, offsets=None, span=None, span_k=0):
    """-> (out bases, out offsets uint64[n_index + 1]); an index >= n_reads gives an empty read"""
    src, ln = clips(n_reads, read_len, offsets, span, span_k)
    index = np.asarray(index).astype(np.uint64)
    ok = index < np.uint64(n_reads)
    i = np.where(ok, index, 0).astype(np.int64)
    s = src[i] if n_reads else np.zeros(len(index), np.int64)
    n = np.where(ok, ln[i], 0) if n_reads else np.zeros(len(index), np.int64)
    return _emit(np.asarray(bases), s, n)


def partition_np(bases, n_reads, read_len, labels, offsets=None):
    """-> (out bases, out offsets, index uint64, distinct labels int64 ascending, group_offsets int64[G + 1]): the reads of every
    non-negative label, grouped by label ascending, source order within a group"""
    labels = np.asarray(labels).astype(np.int64)[:n_reads]
    order = np.argsort(labels, kind="stable")
    order = order[labels[order] >= 0]
    distinct, counts = np.unique(labels[order], return_counts=True)
    group_offsets = np.zeros(len(distinct) + 1, np.int64)
    group_offsets[1:] = np.cumsum(counts)
    out, off = gather_np(bases, n_reads, read_len, order.astype(np.uint64), offsets)
    return out, off, order.astype(np.uint64), distinct, group_offsets
