"""tests/merge_np.py, the host reference of kmx_reads_pair_merge, pinned on the CPU against a literal per-position loop that follows
include/kmx.h sentence by sentence; the random batches it is pinned on are shown to contain every class, every sign of d, every
relation of I to L1 and every reason not to merge.  And the places the new symbol has to appear in."""
import os

import numpy as np

from tests import merge_np as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA = np.frombuffer(b"ACGTacgtN.", np.uint8)
VALID = set(b"ACGTacgt")
COMP = dict(zip(b"ACGTacgt", b"TGCAtgca"))


def loop_pair(m1, m2, q1, q2, I, phred, cap):
    """the merged read of one pair that merges, position by position -> (bases, quality bytes, row, the classes seen)"""
    L1, L2 = len(m1), len(m2)
    d = I - L2
    out, outq, seen = bytearray(), bytearray(), set()
    n = n_dis = n_taken = n_tie = n_one = n_none = 0
    for i in range(I):
        in_x, in_y = i < L1, i >= max(d, 0)
        assert in_x or in_y
        xb = m1[i] if in_x else None
        j = i - d
        yb = COMP.get(m2[L2 - 1 - j], ord("N")) if in_y else None
        if not (in_x and in_y):
            out.append(xb if in_x else yb)
            outq.append((q1[i] if in_x else q2[L2 - 1 - j]) if q1 is not None else 0)
            continue
        n += 1
        bx, by = (q1[i], q2[L2 - 1 - j]) if q1 is not None else (0, 0)
        qx = bx - phred if q1 is not None and bx >= phred else 0
        qy = by - phred if q1 is not None and by >= phred else 0
        vx, vy = xb in VALID, yb in VALID
        if vx and vy and chr(xb).upper() == chr(yb).upper():
            b, q = xb, qx + qy
            seen.add("agree_capped" if q >= cap else "agree")
        elif vx and vy:
            n_dis += 1
            if qy > qx:
                b, q = yb, qy - qx
                n_taken += 1
                seen.add("dis_mate2")
            else:
                b, q = xb, qx - qy
                seen.add("dis_tie" if qx == qy else "dis_mate1")
            n_tie += qx == qy
        elif vx or vy:
            b, q = (xb, qx) if vx else (yb, qy)
            n_one += 1
            seen.add("one_x" if vx else "one_y")
        else:
            b, q = ord("N"), 0
            n_none += 1
            seen.add("none")
        out.append(b)
        outq.append(phred + min(q, cap))
    assert n == min(L1, I) - max(d, 0)
    return bytes(out), bytes(outq), [I, n | n_dis << 32, n_taken | n_tie << 32, n_one | n_none << 32], seen


def loop_batch(reads1, reads2, quals1, quals2, insert, phred, cap):
    seen, bases, quals, offsets, rows = set(), b"", b"", [0], []
    for r, (m1, m2) in enumerate(zip(reads1, reads2)):
        L1, L2, I = len(m1), len(m2), int(insert[r])
        if not (1 <= L1 <= 1024 and 1 <= L2 <= 1024):
            seen.add("no_empty" if min(L1, L2) == 0 else "no_long")
        elif I == 0:
            seen.add("no_zero")
        elif I >= L1 + L2:
            seen.add("no_large")
        else:
            b, q, row, s = loop_pair(m1, m2, quals1[r] if quals1 else None, quals2[r] if quals2 else None, I, phred, cap)
            d = I - L2
            seen |= s | {"d<0" if d < 0 else "d==0" if d == 0 else "d>0", "I<L1" if I < L1 else "I==L1" if I == L1 else "I>L1"}
            bases, quals = bases + b, quals + q
            rows.append(row)
            offsets.append(offsets[-1] + I)
            continue
        rows.append([0, 0, 0, 0])
        offsets.append(offsets[-1])
    return bases, quals, offsets, rows, seen


def random_batch(rng, n, phred):
    """mates over ACGTacgtN. with quality bytes from below phred up; the insert words cover every relation to the lengths"""
    lens = [(int(rng.integers(1, 40)), int(rng.integers(1, 40))) for _ in range(n)]
    lens[3], lens[4], lens[5], lens[6] = (0, 12), (9, 0), (1025, 30), (30, 1030)
    reads1 = [rng.choice(ALPHA, a).astype(np.uint8).tobytes() for a, _ in lens]
    reads2 = [rng.choice(ALPHA, b).astype(np.uint8).tobytes() for _, b in lens]
    quals1 = [rng.integers(phred - 3, phred + 45, a).astype(np.uint8).tobytes() for a, _ in lens]
    quals2 = [rng.integers(phred - 3, phred + 45, b).astype(np.uint8).tobytes() for _, b in lens]
    insert = np.zeros(n, np.uint64)
    for r, (a, b) in enumerate(lens):
        pick = r % 8
        insert[r] = (0, a + b, a + b + 7, b, a, 1 << 40)[pick] if pick < 6 else int(rng.integers(1, max(a + b, 2)))
    insert[7] = np.uint64(M.M64)
    return reads1, reads2, quals1, quals2, insert


def as_batch(reads, first=0):
    off = (np.concatenate([[0], np.cumsum([len(r) for r in reads])]) + first).astype(np.uint64)
    return np.frombuffer(b"." * first + b"".join(reads), np.uint8), off


def test_reference_equals_the_literal_loop_and_the_batches_hold_every_class():
    rng = np.random.default_rng(41)
    seen = set()
    for phred, cap in ((33, 41), (64, 10), (33, 0), (0, 255)):
        reads1, reads2, quals1, quals2, insert = random_batch(rng, 160, max(phred, 3))
        want_b, want_q, want_off, want_rows, s = loop_batch(reads1, reads2, quals1, quals2, insert, phred, cap)
        if cap == 41:
            seen |= s
        (b1, o1), (b2, o2) = as_batch(reads1, 5), as_batch(reads2, 2)
        (q1, _), (q2, _) = as_batch(quals1, 5), as_batch(quals2, 2)
        got_b, got_q, got_off, got_rows = M.reads_pair_merge_np(b1, b2, len(reads1), 0, 0, insert, q1, q2, o1, o2, phred, cap)
        assert got_b.tobytes() == want_b and got_q.tobytes() == want_q
        assert got_off.tolist() == want_off and got_rows.tolist() == want_rows
        # without quality bytes: every q is 0, mate 1 wins every DIS
        want_b, _, want_off, want_rows, _ = loop_batch(reads1, reads2, None, None, insert, phred, cap)
        got_b, got_q, got_off, got_rows = M.reads_pair_merge_np(b1, b2, len(reads1), 0, 0, insert, None, None, o1, o2, phred, cap)
        assert got_q is None and got_b.tobytes() == want_b and got_off.tolist() == want_off and got_rows.tolist() == want_rows
        assert not any(row[M.RM_TAKEN] & 0xFFFFFFFF for row in want_rows)
    assert seen == {"agree", "agree_capped", "dis_mate1", "dis_mate2", "dis_tie", "one_x", "one_y", "none", "d<0", "d==0", "d>0", "I<L1", "I==L1",
                    "I>L1", "no_zero", "no_large", "no_long", "no_empty"}, seen


def test_uniform_mates_and_the_insert_as_int64_bits():
    rng = np.random.default_rng(42)
    n, L1, L2 = 30, 20, 17
    b1, b2 = rng.choice(ALPHA, n * L1).astype(np.uint8), rng.choice(ALPHA, n * L2).astype(np.uint8)
    q1, q2 = rng.integers(30, 80, n * L1).astype(np.uint8), rng.integers(30, 80, n * L2).astype(np.uint8)
    insert = rng.integers(0, L1 + L2 + 3, n).astype(np.uint64)
    insert[2] = np.uint64(M.M64 - 5)
    reads1, reads2 = [b1[r * L1:(r + 1) * L1].tobytes() for r in range(n)], [b2[r * L2:(r + 1) * L2].tobytes() for r in range(n)]
    quals1, quals2 = [q1[r * L1:(r + 1) * L1].tobytes() for r in range(n)], [q2[r * L2:(r + 1) * L2].tobytes() for r in range(n)]
    want_b, want_q, want_off, want_rows, _ = loop_batch(reads1, reads2, quals1, quals2, insert, 33, 41)
    got_b, got_q, got_off, got_rows = M.reads_pair_merge_np(b1, b2, n, L1, L2, insert.view(np.int64), q1, q2)
    assert got_b.tobytes() == want_b and got_q.tobytes() == want_q and got_off.tolist() == want_off and got_rows.tolist() == want_rows


def test_error_free_mates_of_a_planted_fragment_merge_to_the_fragment():
    rng = np.random.default_rng(43)
    for L1, L2, I in ((150, 150, 200), (150, 150, 90), (100, 150, 120), (150, 100, 249), (30, 30, 1), (64, 64, 64)):
        frag = rng.choice(np.frombuffer(b"ACGT", np.uint8), I).astype(np.uint8).tobytes()
        junk1, junk2 = rng.choice(ALPHA, L1).astype(np.uint8).tobytes(), rng.choice(ALPHA, L2).astype(np.uint8).tobytes()
        m1, m2 = (frag + junk1)[:L1], (M.revcomp(frag) + junk2)[:L2]
        q1, q2 = rng.integers(35, 75, L1).astype(np.uint8), rng.integers(35, 75, L2).astype(np.uint8)
        out, outq, off, rows = M.reads_pair_merge_np(np.frombuffer(m1, np.uint8), np.frombuffer(m2, np.uint8), 1, L1, L2, np.array([I], np.uint64), q1, q2)
        n = min(L1, I) - max(I - L2, 0)
        assert out.tobytes() == frag and off.tolist() == [0, I] and rows[0].tolist() == [I, n, 0, 0]
        assert len(outq) == I and (outq >= 33).all() and (outq <= 33 + 41).all()


def test_the_symbol_is_in_every_layer():
    from kmers_amd import _lib, build

    name = "kmx_reads_pair_merge"
    assert name in open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 16
    assert name in open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert "kmx_reads_merge.hip" in build.SOURCES
    assert (_lib.RM_LEN, _lib.RM_OVERLAP, _lib.RM_TAKEN, _lib.RM_INVALID, _lib.RM_WORDS) == (M.RM_LEN, M.RM_OVERLAP, M.RM_TAKEN, M.RM_INVALID, M.RM_WORDS)
