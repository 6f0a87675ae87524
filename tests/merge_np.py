"""Host reference of kmx_reads_pair_merge (include/kmx.h, "overlapping mate pairs merged into consensus reads"): what
tests/test_gpu_reads_merge.py compares the device's bases, quality bytes, offsets and row words with.  Vectorised numpy over the
positions of one merged read: lookup tables for the letter and the complement, boolean masks for the four classes.  The definition
-- which pairs merge, what X and Y cover, the classes and their quality rule -- is pinned against a literal per-position loop in
tests/test_merge_np.py.

A batch is (bases uint8[...], offsets[n + 1]) or, for uniform reads, (bases, None) with read_len; quality bytes are laid out as
their bases are."""
import numpy as np

from tests.quality_np import bounds

RM_LEN, RM_OVERLAP, RM_TAKEN, RM_INVALID = range(4)
RM_WORDS = 4
RP_MAX_LEN = 1024
M64 = (1 << 64) - 1

# a byte's letter: 0..3 for Aa Cc Gg Tt, 4 for anything else
_LETTER = np.full(256, 4, np.int64)
for _i, _pair in enumerate((b"Aa", b"Cc", b"Gg", b"Tt")):
    _LETTER[list(_pair)] = _i
# the complement of a byte: the case is kept, any other byte becomes N
_COMP = np.full(256, ord("N"), np.uint8)
_COMP[list(b"ACGTacgt")] = list(b"TGCAtgca")


def merges(L1, L2, insert) -> bool:
    """the pair merges (insert: the word as an unsigned Python integer)"""
    return 1 <= L1 <= RP_MAX_LEN and 1 <= L2 <= RP_MAX_LEN and 0 < insert < L1 + L2


def merge_pair(m1, m2, q1, q2, insert, phred_base=33, q_cap=41):
    """one pair that merges -> (bases uint8[I], quality bytes uint8[I], row as four Python integers); q1 = q2 = None: every q is 0
    and the quality bytes returned are meaningless"""
    m1, m2 = np.asarray(m1, dtype=np.uint8), np.asarray(m2, dtype=np.uint8)
    L1, L2, I = len(m1), len(m2), int(insert)
    d = I - L2
    if q1 is None:
        q1, q2 = np.zeros(L1, np.uint8), np.zeros(L2, np.uint8)
        phred_base = 0
    q1, q2 = np.asarray(q1, dtype=np.uint8), np.asarray(q2, dtype=np.uint8)
    # X and Y on the positions of M: where a mate does not cover, byte 0
    x, xq, y, yq = (np.zeros(I, np.uint8) for _ in range(4))
    x1, y0 = min(L1, I), max(d, 0)
    x[:x1], xq[:x1] = m1[:x1], q1[:x1]
    y[y0:], yq[y0:] = _COMP[m2[::-1]][y0 - d:], q2[::-1][y0 - d:]
    pos = np.arange(I)
    both = (pos < x1) & (pos >= y0)
    vx, vy = _LETTER[x] < 4, _LETTER[y] < 4
    qx = np.maximum(xq.astype(np.int64) - phred_base, 0)
    qy = np.maximum(yq.astype(np.int64) - phred_base, 0)
    agree = both & vx & vy & (_LETTER[x] == _LETTER[y])
    dis = both & vx & vy & ~agree
    one_x, one_y, none = both & vx & ~vy, both & ~vx & vy, both & ~vx & ~vy
    take = dis & (qy > qx)
    from_y = (pos >= x1) | take | one_y
    out = np.where(from_y, y, x)
    out[none] = ord("N")
    q = np.select([agree, dis, one_x, one_y], [qx + qy, np.abs(qx - qy), qx, qy], 0)
    outq = np.where(both, phred_base + np.minimum(q, q_cap), np.where(pos < x1, xq, yq)).astype(np.uint8)
    row = [I, int(both.sum()) | (int(dis.sum()) << 32), int(take.sum()) | (int((dis & (qx == qy)).sum()) << 32),
           int((one_x | one_y).sum()) | (int(none.sum()) << 32)]
    return out.astype(np.uint8), outq, row


def reads_pair_merge_np(bases1, bases2, n_reads, read_len1, read_len2, insert, quals1=None, quals2=None, offsets1=None, offsets2=None,
                        phred_base=33, q_cap=41):
    """-> (bases uint8[n_bases], quality bytes uint8[n_bases] or None, offsets uint64[n_reads + 1], rows uint64[n_reads, 4]);
    `insert`: one word per pair (uint64, or int64 holding the same bits)"""
    bases1, bases2 = np.asarray(bases1, dtype=np.uint8), np.asarray(bases2, dtype=np.uint8)
    insert = np.asarray(insert).astype(np.uint64)
    rows = np.zeros((n_reads, RM_WORDS), np.uint64)
    offsets = np.zeros(n_reads + 1, np.uint64)
    b1, b2 = bounds(n_reads, read_len1, offsets1), bounds(n_reads, read_len2, offsets2)
    parts, qparts = [], []
    for r in range(n_reads):
        (s1, L1), (s2, L2) = b1[r], b2[r]
        I = int(insert[r])
        if merges(L1, L2, I):
            qa = np.asarray(quals1, dtype=np.uint8)[s1:s1 + L1] if quals1 is not None else None
            qb = np.asarray(quals2, dtype=np.uint8)[s2:s2 + L2] if quals2 is not None else None
            out, outq, row = merge_pair(bases1[s1:s1 + L1], bases2[s2:s2 + L2], qa, qb, I, phred_base, q_cap)
            parts.append(out)
            qparts.append(outq)
            rows[r] = np.array(row, dtype=np.uint64)
        else:
            I = 0
        offsets[r + 1] = offsets[r] + np.uint64(I)
    out = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    outq = (np.concatenate(qparts) if qparts else np.zeros(0, np.uint8)) if quals1 is not None else None
    return out, outq, offsets, rows


def revcomp(seq):
    """of a byte string (test helper: planting fragments)"""
    return _COMP[np.frombuffer(bytes(seq), np.uint8)[::-1]].tobytes()
