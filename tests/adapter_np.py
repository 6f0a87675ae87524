"""Host reference of kmx_reads_adapter and kmx_reads_pair_overlap (include/kmx.h, "adapter read-through"): what
tests/test_gpu_reads_adapter.py and tests/test_gpu_pair_overlap.py compare the device's row words with.  Vectorised numpy: a read
against an adapter is a (positions x adapter bases) mismatch matrix over a sliding window, a mate pair an (L1 x L2) match matrix
summed along its diagonals.  The definitions -- the overlap that hangs over the read's end, wildcards, invalid bytes, the integer
error rate, the three tie rules -- are pinned against literal per-position loops in tests/test_adapter_np.py.

A batch is (bases uint8[...], offsets[n + 1]) or, for uniform reads, (bases, None) with read_len."""
import numpy as np

from tests.quality_np import bounds

RA_KEEP, RA_HIT, RA_BASES, RA_HITS = range(4)
RA_WORDS = 4
RP_INSERT, RP_OVERLAP, RP_KEEP1, RP_KEEP2 = range(4)
RP_WORDS = 4
RP_MAX_LEN = 1024
M64 = (1 << 64) - 1

# a byte's letter: 0..3 for Aa Cc Gg Tt, 4 for N / n, 5 for anything else
_LETTER = np.full(256, 5, np.int64)
for _i, _pair in enumerate((b"Aa", b"Cc", b"Gg", b"Tt", b"Nn")):
    _LETTER[list(_pair)] = _i
_COMP = np.array([3, 2, 1, 0, 5, 5], np.int64)   # of a letter; N and the rest stay invalid


def adapter_ok(adapter) -> bool:
    a = np.frombuffer(bytes(adapter), np.uint8)
    return 1 <= len(a) <= 64 and bool((_LETTER[a] <= 4).all())


def adapter_scan(read, adapter):
    """-> (n int64[L], m int64[L]): the overlap and the mismatches of the adapter at every position of the read"""
    r = _LETTER[np.asarray(read, dtype=np.uint8)]
    a = _LETTER[np.frombuffer(bytes(adapter), np.uint8)]
    L, A = len(r), len(a)
    if L == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    n = np.minimum(A, L - np.arange(L))
    win = np.lib.stride_tricks.sliding_window_view(np.concatenate([r, np.full(A - 1, 5, np.int64)]), A)   # [L, A]
    r_acgt = win <= 3
    mism = (a[None, :] != 4) & ~(r_acgt & (win == a[None, :])) & (np.arange(A)[None, :] < n[:, None])
    return n, mism.sum(axis=1)


def adapter_row(read, adapters, min_overlap, err_num, err_den):
    """the four words of one read (Python integers)"""
    L = len(read)
    best = None   # (p, a, n, m)
    hits = 0
    for ai, ad in enumerate(adapters):
        n, m = adapter_scan(read, ad)
        hit = (n >= min_overlap) & (m * int(err_den) <= int(err_num) * n)
        ps = np.nonzero(hit)[0]
        if len(ps):
            hits |= 1 << ai
            p = int(ps[0])
            if best is None or p < best[0]:
                best = (p, ai, int(n[p]), int(m[p]))
    row = [0] * RA_WORDS
    row[RA_KEEP] = (best[0] if best else L) << 32
    row[RA_HIT] = ((best[1] + 1) | (best[2] << 16) | (best[3] << 32)) if best else 0
    row[RA_BASES] = L
    row[RA_HITS] = hits
    return row


def reads_adapter_np(bases, n_reads, read_len, adapters, min_overlap=3, err_num=1, err_den=10, offsets=None):
    """-> rows uint64[n_reads, 4]"""
    bases = np.asarray(bases, dtype=np.uint8)
    rows = np.zeros((n_reads, RA_WORDS), np.uint64)
    for r, (s, L) in enumerate(bounds(n_reads, read_len, offsets)):
        rows[r] = np.array(adapter_row(bases[s:s + L], adapters, min_overlap, err_num, err_den), dtype=np.uint64)
    return rows


def pair_scan(mate1, mate2):
    """-> (n int64[L1 + L2 - 1], m likewise), entry t for the shift d = t - (L2 - 1): the insert size is t + 1"""
    x = _LETTER[np.asarray(mate1, dtype=np.uint8)]
    y = _COMP[_LETTER[np.asarray(mate2, dtype=np.uint8)]][::-1]
    L1, L2 = len(x), len(y)
    if L1 == 0 or L2 == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    match = (x[:, None] <= 3) & (x[:, None] == y[None, :])                   # X[i] against Y[j]: d = i - j
    t = (np.arange(L1)[:, None] - np.arange(L2)[None, :]) + (L2 - 1)
    same = np.bincount(t.ravel(), weights=match.ravel(), minlength=L1 + L2 - 1).astype(np.int64)
    d = np.arange(L1 + L2 - 1) - (L2 - 1)
    n = np.minimum(L1, d + L2) - np.maximum(0, d)
    return n, n - same


def pair_row(mate1, mate2, min_overlap, max_mism, err_num, err_den):
    L1, L2 = len(mate1), len(mate2)
    row = [0, 0, L1 << 32, L2 << 32]
    if L1 > RP_MAX_LEN or L2 > RP_MAX_LEN:
        return row
    n, m = pair_scan(mate1, mate2)
    hit = (n >= min_overlap) & (m <= max_mism) & (m * int(err_den) <= int(err_num) * n)
    ts = np.nonzero(hit)[0]
    if len(ts):
        nmax = int(n[ts].max())
        t = int(ts[n[ts] == nmax].max())
        ins = t + 1
        row = [ins, nmax | (int(m[t]) << 32), min(L1, ins) << 32, min(L2, ins) << 32]
    return row


def reads_pair_overlap_np(bases1, bases2, n_reads, read_len1, read_len2, offsets1=None, offsets2=None, min_overlap=30, max_mism=5, err_num=1,
                          err_den=5):
    """-> rows uint64[n_reads, 4]"""
    bases1, bases2 = np.asarray(bases1, dtype=np.uint8), np.asarray(bases2, dtype=np.uint8)
    rows = np.zeros((n_reads, RP_WORDS), np.uint64)
    b1, b2 = bounds(n_reads, read_len1, offsets1), bounds(n_reads, read_len2, offsets2)
    for r in range(n_reads):
        (s1, L1), (s2, L2) = b1[r], b2[r]
        rows[r] = np.array(pair_row(bases1[s1:s1 + L1], bases2[s2:s2 + L2], min_overlap, max_mism, err_num, err_den), dtype=np.uint64)
    return rows


def revcomp(seq):
    """of a byte string over ACGT (test helper: planting overlaps)"""
    return bytes(seq)[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))
