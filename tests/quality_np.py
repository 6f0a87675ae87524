"""Host reference of kmx_fastx_parse_quals and kmx_reads_quality (include/kmx.h, "FASTQ qualities"): what tests/test_gpu_fastx_quals.py
and tests/test_gpu_reads_quality.py compare the device's bytes and row words with.  The row words that have more than one plausible
reading -- the Mott span with its two tie rules, the leftmost longest run, the window count -- are pinned against brute-force
O(L^2) pure-Python searches in tests/test_quality_np.py.

A batch is (bases uint8[...], offsets[n + 1]) or, for uniform reads, (bases, None) with read_len; quals has the layout of bases."""
import numpy as np

RQ_BASES, RQ_LOW, RQ_QSUM, RQ_WEIGHT, RQ_MINMAX, RQ_TRIM, RQ_RUN, RQ_WINDOWS = range(8)
RQ_WORDS = 8
_ACGT = np.zeros(256, bool)
_ACGT[list(b"ACGTacgt")] = True
M64 = (1 << 64) - 1


def fastq_quals(text: bytes):
    """-> (quals uint8[n_bytes], qoffsets uint64[n + 1]): line i % 4 == 3 of the text, every '\\r' dropped; what follows the last
    newline is a line only if it has a byte"""
    text = bytes(text)
    if not text:
        return np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    if text[:1] != b"@":
        raise ValueError("not a FASTQ text")
    lines = text.split(b"\n")
    if text.endswith(b"\n"):
        lines.pop()
    quals = [ln.replace(b"\r", b"") for ln in lines[3::4]]
    off = np.zeros(len(quals) + 1, np.uint64)
    if quals:
        off[1:] = np.cumsum([len(q) for q in quals], dtype=np.uint64)
    return np.frombuffer(b"".join(quals), dtype=np.uint8).copy(), off


def first_mismatch(qoffsets, read_offsets):
    """the smallest r whose two lengths differ, or 2^64 - 1"""
    n = len(qoffsets) - 1
    a = np.diff(np.asarray(qoffsets).astype(np.int64))
    b = np.diff(np.asarray(read_offsets).astype(np.int64))[:n]
    bad = np.nonzero(a != b)[0]
    return int(bad[0]) if len(bad) else M64


def ee_weights(phred=33):
    """the default weight table, 256 words by the RAW quality byte: round(2^32 * 10^(-q / 10)) for q = max(byte - phred, 0)"""
    q = np.maximum(np.arange(256, dtype=np.int64) - int(phred), 0)
    return np.round(2.0**32 * 10.0 ** (-q / 10.0)).astype(np.uint64)


def q_values(qbytes, phred):
    qb = np.asarray(qbytes).astype(np.int64)
    return np.where(qb >= phred, qb - phred, 0)


def mott_span(q, trim_q):
    """(start, len) of the trim span of kmx.h, one forward pass: the running minimum of the prefix sums with its LAST index, the
    first b at which P_b - min reaches its overall maximum"""
    P, M, A = 0, 0, 0
    V, bs, as_ = 0, 0, 0
    for i, x in enumerate(q):
        P += int(x) - trim_q
        b = i + 1
        if P <= M:
            M, A = P, b
        if P - M > V:
            V, bs, as_ = P - M, b, A
    return (as_, bs - as_) if V > 0 else (0, 0)


def longest_run(good):
    """(start, len) of the longest run of True, the leftmost of equal ones; (0, 0) if there is none"""
    best, start, run = (0, 0), 0, 0
    for i, g in enumerate(good):
        if g:
            if run == 0:
                start = i
            run += 1
            if run > best[1]:
                best = (start, run)
        else:
            run = 0
    return best


def good_windows(good, k):
    if k == 0:
        return 0
    n, run = 0, 0
    for g in good:
        run = run + 1 if g else 0
        n += run >= k
    return n


def read_row(bases, qbytes, phred, min_q, trim_q, k, weights=None):
    """the eight words of one read (Python integers)"""
    L = len(bases)
    q = q_values(qbytes, phred)
    low = q < min_q
    good = _ACGT[np.asarray(bases, dtype=np.uint8)] & ~low
    row = [0] * RQ_WORDS
    row[RQ_BASES] = L
    row[RQ_LOW] = int(low.sum())
    row[RQ_QSUM] = int(q.sum())
    if weights is not None:
        row[RQ_WEIGHT] = sum(int(weights[int(b)]) for b in qbytes) & M64
    row[RQ_MINMAX] = (int(q.min()) | (int(q.max()) << 32)) if L else 0
    s, n = mott_span(q.tolist(), trim_q)
    row[RQ_TRIM] = s | (n << 32)
    s, n = longest_run(good.tolist())
    row[RQ_RUN] = s | (n << 32)
    row[RQ_WINDOWS] = good_windows(good.tolist(), k)
    return row


def bounds(n_reads, read_len, offsets):
    """(first byte, length) of every read, Python integers; 2^31 bases or more, or descending offsets: length 0"""
    out = []
    for r in range(n_reads):
        if offsets is None:
            a, L = r * read_len, read_len
        else:
            a, L = int(offsets[r]), int(offsets[r + 1]) - int(offsets[r])
        out.append((a, 0 if (L < 0 or L >= 2**31) else L))
    return out


def reads_quality_np(bases, quals, n_reads, read_len, offsets=None, phred=33, min_q=0, trim_q=0, k=0, weights=None):
    """-> (masked uint8 like bases: bytes outside the reads unchanged, rows uint64[n_reads, 8])"""
    bases = np.asarray(bases, dtype=np.uint8)
    quals = np.asarray(quals, dtype=np.uint8)
    masked = bases.copy()
    rows = np.zeros((n_reads, RQ_WORDS), np.uint64)
    for r, (a, L) in enumerate(bounds(n_reads, read_len, offsets)):
        b, qb = bases[a:a + L], quals[a:a + L]
        masked[a:a + L] = np.where(q_values(qb, phred) < min_q, ord("N"), b)
        rows[r] = np.array(read_row(b, qb, phred, min_q, trim_q, k, weights), dtype=np.uint64)
    return masked, rows


def expected_errors_np(rows):
    return rows[:, RQ_WEIGHT].astype(np.float64) / 2.0**32
