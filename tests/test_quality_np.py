"""tests/quality_np.py pinned against brute force: the Mott span by its definition in include/kmx.h (every pair a <= b, then the two
tie rules spelled out), the longest run by trying every interval, the window count by testing every window.  Reads of up to 40
bases over three quality values, so equal sums, plateaus and equal runs are everywhere.  No GPU."""
import numpy as np

from tests import quality_np as Q


def brute_mott(q, t):
    L = len(q)
    P = [0]
    for x in q:
        P.append(P[-1] + x - t)
    V = max(P[b] - P[a] for b in range(L + 1) for a in range(b + 1))
    if V == 0:
        return 0, 0
    bs = min(b for b in range(L + 1) if max(P[b] - P[a] for a in range(b + 1)) == V)
    as_ = max(a for a in range(bs) if P[bs] - P[a] == V)
    return as_, bs - as_


def brute_run(good):
    L = len(good)
    best = (0, 0)
    for n in range(L, 0, -1):
        for s in range(0, L - n + 1):
            if all(good[s:s + n]):
                return s, n
    return best


def brute_windows(good, k):
    if k == 0:
        return 0
    return sum(1 for s in range(0, len(good) - k + 1) if all(good[s:s + k]))


def _cases():
    rng = np.random.default_rng(20240607)
    out = [[], [5], [0], [9]]
    for L in range(1, 41):
        for _ in range(12):
            out.append(rng.choice([0, 5, 9], L).tolist())
    return out


def test_mott_span_against_brute_force():
    for q in _cases():
        for t in (0, 4, 5, 6, 9, 10):
            assert Q.mott_span(q, t) == brute_mott(q, t), (q, t)


def test_mott_span_ends_on_bases_above_the_threshold():
    for q in _cases():
        for t in (4, 5, 8):
            s, n = Q.mott_span(q, t)
            if n:
                assert q[s] > t and q[s + n - 1] > t, (q, t, s, n)
            else:
                assert all(x <= t for x in q)


def test_mott_tie_rules_on_plateaus():
    # a zero-sum stretch before the span is left out (a* is the LARGEST a), one after it too (b* is the SMALLEST b)
    assert Q.mott_span([9, 1, 9, 5, 5, 9, 1], 5) == (2, 4)        # P = 0 4 0 4 4 4 8 4: the zero-sum [0, 2) before the span is left out
    assert Q.mott_span([9, 1, 9], 5) == (0, 1)                    # P = 0 4 0 4: V is reached at b = 1 and again at b = 3; the first wins
    assert Q.mott_span([5, 5, 9, 9, 5, 5], 5) == (2, 2)
    assert Q.mott_span([1, 9, 1, 9], 5) == (1, 1)
    assert Q.mott_span([5] * 7, 5) == (0, 0)                     # V == 0


def test_longest_run_and_windows_against_brute_force():
    rng = np.random.default_rng(7)
    for L in range(0, 41):
        for _ in range(8):
            good = (rng.random(L) < 0.7).tolist()
            assert Q.longest_run(good) == brute_run(good), good
            for k in (0, 1, 2, 5, L, L + 1):
                assert Q.good_windows(good, k) == brute_windows(good, k), (good, k)


def test_read_row_words():
    bases = np.frombuffer(b"ACGTNacgtX", np.uint8)
    quals = np.frombuffer(bytes([33 + 9, 33 + 9, 33 + 0, 33 + 9, 33 + 9, 33 + 9, 33 + 9, 33 + 5, 20, 0xF0]), np.uint8)
    w = np.arange(256, dtype=np.uint64) * np.uint64(3)
    row = Q.read_row(bases, quals, 33, 5, 5, 2, w)
    q = [9, 9, 0, 9, 9, 9, 9, 5, 0, 0xF0 - 33]
    assert row[Q.RQ_BASES] == 10 and row[Q.RQ_LOW] == 2 and row[Q.RQ_QSUM] == sum(q)
    assert row[Q.RQ_WEIGHT] == 3 * int(quals.astype(np.int64).sum())
    assert row[Q.RQ_MINMAX] == 0 | ((0xF0 - 33) << 32)
    # good: A C . T . a c g . .  (base 2 and 8 low, N and X not ACGT)
    assert row[Q.RQ_RUN] == 5 | (3 << 32)
    assert row[Q.RQ_WINDOWS] == 1 + 2
    assert row[Q.RQ_TRIM] == (lambda s, n: s | (n << 32))(*brute_mott(q, 5))
    masked, rows = Q.reads_quality_np(bases, quals, 2, 5, None, 33, 5, 5, 2, w)
    assert masked.tobytes() == b"ACNTNacgNX" and rows.shape == (2, 8) and int(rows[0, Q.RQ_BASES]) == 5


def test_fastq_quals_lines():
    assert Q.fastq_quals(b"")[1].tolist() == [0]
    for text, want in [(b"@x", []), (b"@x\nAC\n+\n", []), (b"@x\nAC\n+\nI", [b"I"]), (b"@x\nAC\n+\n\n", [b""]),
                       (b"@x\r\nAC\r\n+\r\n@>\r\n@y\nA\n+\n+", [b"@>", b"+"])]:
        q, off = Q.fastq_quals(text)
        assert q.tobytes() == b"".join(want) and off.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in want])]).tolist(), text
    assert Q.first_mismatch([0, 2, 4], [0, 2, 4]) == Q.M64 and Q.first_mismatch([0, 2, 4, 5], [0, 2, 5, 6]) == 1
