"""Host reference of kmx_reads_dedup, written from the contract in include/kmx.h: codes, the fingerprint H, the pair fingerprint P,
keys, rank, heads and the decision by direct comparison of code sequences.  Plain Python integers (mod 2^64 by masking): slow and
obvious.  A read is a bytes object; a batch is a list of them.  (No fixtures, no device code.)"""
import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
WORDS, REP, COUNT, FLAGS, HASH = 4, 0, 1, 2, 3
F_KEPT, F_FLIPPED, F_COLLISION, F_OTHER = 1, 2, 4, 8
S_KEPT, S_DROPPED, S_LARGEST, S_COLLISIONS = range(4)

_CODE = bytearray([4]) * 256
for _i, _pair in enumerate((b"Aa", b"Cc", b"Gg", b"Tt")):
    for _b in _pair:
        _CODE[_b] = _i
_CODE = bytes(_CODE)
_COMP = bytes([3, 2, 1, 0, 4]) + bytes(251)


def fmix(x):
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 33
    return x


def codes(read):
    """the code sequence of a read, one byte per code"""
    return bytes(read).translate(_CODE)


def rc(code_seq):
    return code_seq[::-1].translate(_COMP)


def revcomp_bytes(read):
    """the reverse complement of a read as bytes (ACGT, case kept; any other byte stays what it is)"""
    t = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    return bytes(read)[::-1].translate(t)


def H(code_seq):
    L = len(code_seq)
    total = 0
    for p in range((L + 3) // 4):
        v = 0
        for j in range(4):
            q = 4 * p + j
            v |= (code_seq[q] if q < L else 0xF) << (4 * j)
        total += fmix((((p << 16) | v) + G) & M64)
    return fmix((total & M64) ^ ((L * G) & M64))


def P(x, y):
    return fmix((fmix((x + G) & M64) + y) & M64)


def dedup(reads, mates=None, strand=False, score=None, hash_bits=64):
    """-> (rows uint64[n, 4], keep uint8[n], summary uint64[4]) as kmx_reads_dedup defines them"""
    n = len(reads)
    memo = {}

    def h_of(c):
        if c not in memo:
            memo[c] = H(c)
        return memo[c]

    c1 = [codes(r) for r in reads]
    c2 = [codes(r) for r in mates] if mates is not None else None
    sh = 64 - hash_bits
    key, other = [0] * n, [False] * n
    for r in range(n):
        if c2 is None:
            fa, fb = h_of(c1[r]) >> sh, h_of(rc(c1[r])) >> sh
        else:
            x, y = h_of(c1[r]), h_of(c2[r])
            fa, fb = P(x, y) >> sh, P(y, x) >> sh
        if strand:
            key[r], other[r] = min(fa, fb), fb < fa
        else:
            key[r] = fa
    s = [0] * n if score is None else [min(int(v), (1 << 32) - 1) for v in score]
    head = {}
    for r in sorted(range(n), key=lambda r: (-s[r], r)):
        head.setdefault(key[r], r)

    def same(r, h):
        return c1[r] == c1[h] and (c2 is None or c2[r] == c2[h])

    def flipped(r, h):
        if not strand:
            return False
        return rc(c1[r]) == c1[h] if c2 is None else (c1[r] == c2[h] and c2[r] == c1[h])

    rows = np.zeros((n, WORDS), np.uint64)
    keep = np.ones(n, np.uint8)
    count = [1] * n
    collisions = 0
    for r in range(n):
        h = head[key[r]]
        fl = F_OTHER if other[r] else 0
        rep = r
        if h != r:
            sm = same(r, h)
            fp = (not sm) and flipped(r, h)
            if sm or fp:
                rep, keep[r], count[r] = h, 0, 0
                count[h] += 1
                fl |= F_FLIPPED if fp else 0
            else:
                fl |= F_COLLISION
                collisions += 1
        rows[r, REP], rows[r, FLAGS], rows[r, HASH] = rep, fl | (F_KEPT if keep[r] else 0), key[r]
    rows[:, COUNT] = count
    kept = int(keep.sum())
    summary = np.array([kept, n - kept, max(count) if n else 0, collisions], np.uint64)
    return rows, keep, summary


def canonical_string(read, mate=None, strand=False):
    """what a plain dictionary dedup keys on: the code sequence, or with strand the smaller of it and the other strand's"""
    if mate is None:
        c = codes(read)
        return min(c, rc(c)) if strand else c
    a, b = codes(read), codes(mate)
    return min((a, b), (b, a)) if strand else (a, b)


def dict_dedup(reads, mates=None, strand=False):
    """keep bytes of a first-occurrence dictionary dedup on canonical strings"""
    seen, keep = set(), np.zeros(len(reads), np.uint8)
    for r in range(len(reads)):
        c = canonical_string(reads[r], None if mates is None else mates[r], strand)
        if c not in seen:
            seen.add(c)
            keep[r] = 1
    return keep
