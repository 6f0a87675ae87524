"""Host reference of kmx_reads_complexity (include/kmx.h, "poly-X ends, base composition, low complexity"): what
tests/test_gpu_reads_complexity.py compares the device's row words and masked bytes with.  Numpy where it is cheap: the mismatches
of every suffix are one reversed running sum, a head is the tail of the reversed read, a window's triplet counts one bincount.
The definitions -- the rate rule, the score and its two tie rules, the meeting ends, the windows, the counted triplets -- are
pinned against literal loops in tests/test_complexity_np.py.

A batch is (bases uint8[...], offsets[n + 1]) or, for uniform reads, (bases, None) with read_len."""
import numpy as np

from tests.quality_np import bounds

RX_KEEP, RX_BASES, RX_TAIL, RX_HEAD, RX_AC, RX_GT, RX_DIFF, RX_DUST = range(8)
RX_WORDS = 8
M64 = (1 << 64) - 1
DUST_NEVER = 1891   # S of a full window of one letter: 62 * 61 / 2

# a byte's letter: 0..3 for Aa Cc Gg Tt (the bit index of the base masks), 4 for anything else
_LETTER = np.full(256, 4, np.int64)
for _i, _pair in enumerate((b"Aa", b"Cc", b"Gg", b"Tt")):
    _LETTER[list(_pair)] = _i


def letters_mask(letters) -> int:
    """"G" -> 4, "ACGT" -> 15, "" -> 0 (either case)"""
    m = 0
    for ch in letters:
        m |= 1 << "ACGT".index(ch.upper())
    return m


def n_windows(L: int) -> int:
    return 0 if L == 0 else 1 if L <= 64 else -(-(L - 64) // 32) + 1


def poly_tail(letter, mask, min_len, num, den, penalty):
    """letter: int64[L] of _LETTER -> (t, bit index + 1) of the read's tail, (0, 0) without one"""
    L = len(letter)
    best = (None, 0, 0)   # (s, n, bit + 1)
    n = L - np.arange(L)
    for x in range(4):
        if not (mask >> x) & 1:
            continue
        is_x = letter == x
        m = np.cumsum((~is_x)[::-1])[::-1]
        ok = np.nonzero(is_x & (n >= min_len) & (m * int(den) <= int(num) * n))[0]
        if not len(ok):
            continue
        s = n[ok] - (int(penalty) + 1) * m[ok]
        p = ok[s == s.max()][0]    # of equal scores the longest: the smallest p
        cand = (int(n[p] - (int(penalty) + 1) * m[p]), int(n[p]), x + 1)
        if best[0] is None or (cand[0], cand[1]) > (best[0], best[1]):
            best = cand
    return best[1], best[2]


def window_scores(letter):
    """-> S_j of every window, int64[W]"""
    L = len(letter)
    W = n_windows(L)
    S = np.zeros(W, np.int64)
    if L < 3:
        return S
    valid = letter < 4
    counted = valid[:-2] & valid[1:-1] & valid[2:]
    spell = letter[:-2] + 4 * letter[1:-1] + 16 * letter[2:]
    for j in range(W):
        lo, hi = 32 * j, min(32 * j + 64, L)
        if hi - lo < 3:
            continue
        c = np.bincount(spell[lo:hi - 2][counted[lo:hi - 2]], minlength=64)
        S[j] = int((c * (c - 1) // 2).sum())
    return S


def complexity_row(read, tail_bases, head_bases, min_len, num, den, penalty, dust_max):
    """-> (the eight words of one read as Python integers, the masked read uint8[L])"""
    read = np.asarray(read, dtype=np.uint8)
    L = len(read)
    letter = _LETTER[read]
    t, tx = poly_tail(letter, tail_bases, min_len, num, den, penalty) if tail_bases else (0, 0)
    h, hx = poly_tail(letter[::-1], head_bases, min_len, num, den, penalty) if head_bases else (0, 0)
    row = [0] * RX_WORDS
    row[RX_KEEP] = 0 if h + t >= L else h | ((L - h - t) << 32)
    row[RX_BASES] = L
    row[RX_TAIL] = t | (tx << 32)
    row[RX_HEAD] = h | (hx << 32)
    cnt = np.bincount(letter, minlength=5)
    row[RX_AC] = int(cnt[0]) | (int(cnt[1]) << 32)
    row[RX_GT] = int(cnt[2]) | (int(cnt[3]) << 32)
    pair = (letter[:-1] < 4) & (letter[1:] < 4)
    row[RX_DIFF] = int((pair & (letter[:-1] != letter[1:])).sum()) | (int(pair.sum()) << 32)
    S = window_scores(letter)
    dusty = S > int(dust_max)
    row[RX_DUST] = (int(S.max()) | (int(dusty.sum()) << 32)) if len(S) else 0
    masked = read.copy()
    for j in np.nonzero(dusty)[0]:
        masked[32 * j:32 * j + 64] = ord("N")
    return row, masked


def reads_complexity_np(bases, n_reads, read_len, tail_bases=4, head_bases=0, min_len=10, num=1, den=10, penalty=2, dust_max=122, offsets=None):
    """-> (rows uint64[n_reads, 8], masked uint8 like bases: bytes outside the reads unchanged)"""
    bases = np.asarray(bases, dtype=np.uint8)
    masked = bases.copy()
    rows = np.zeros((n_reads, RX_WORDS), np.uint64)
    for r, (s, L) in enumerate(bounds(n_reads, read_len, offsets)):
        row, m = complexity_row(bases[s:s + L], tail_bases, head_bases, min_len, num, den, penalty, dust_max)
        rows[r] = np.array(row, dtype=np.uint64)
        masked[s:s + L] = m
    return rows, masked


def keep_span(rows):
    """-> (start int64[n], len int64[n]) of RX_KEEP"""
    w = rows[:, RX_KEEP]
    return (w & np.uint64(0xFFFFFFFF)).astype(np.int64), (w >> np.uint64(32)).astype(np.int64)


def gc_content_np(rows):
    a, c = rows[:, RX_AC] & np.uint64(0xFFFFFFFF), rows[:, RX_AC] >> np.uint64(32)
    g, t = rows[:, RX_GT] & np.uint64(0xFFFFFFFF), rows[:, RX_GT] >> np.uint64(32)
    tot = (a + c + g + t).astype(np.float64)
    return np.where(tot > 0, (c + g).astype(np.float64) / np.maximum(tot, 1), 0.0)
