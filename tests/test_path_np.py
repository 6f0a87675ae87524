"""The host reference of the read paths (tests/path_np.py), pinned on the CPU against brute force over Python strings.

The brute force never sees a table index, a place or an oriented node.  It spells the unitigs (tests/unitig_np.sequences_np), notes
for every k-mer string of every unitig string where it stands -- (u, q) -- and reads a window w of a read as (u, q, d): d = 0 if w
is the unitig's own k-mer there, 1 if it is its reverse complement (a palindrome is both: the definition says 1).  Two consecutive
windows of a read belong to one segment iff they stand in the same unitig, read in the same direction, at neighbouring positions in
that direction.  A unitig string has no position before 0 or behind its end, so a run cannot cross a unitig boundary or the written
start of a cycle without breaking this rule.  No GPU, no oracle, no library."""
import numpy as np
import pytest

from tests import path_np
from tests.test_unitig_np import HAIRPINS, LETTERS, Graph, _kmers_of, _random_seq, _rc, _val

KS = (5, 6, 9)


def windows_of(reads, k):
    """canonical words ((windows,) or (windows, 2) uint64), flags and window offsets of reads given as strings"""
    canon, flags, wo = [], [], [0]
    for read in reads:
        for w in _kmers_of(read, k) if len(read) >= k else []:
            if all(ch in LETTERS for ch in w):
                fw, rc = _val(w), _val(_rc(w))
                canon.append(min(fw, rc))
                flags.append(1 | (2 if fw < rc else 0))
            else:
                canon.append(0)
                flags.append(0)
        wo.append(len(canon))
    if k <= 31:
        c = np.array(canon, np.uint64).reshape(-1)
    else:
        c = np.array([[v & (2**64 - 1), v >> 64] for v in canon], np.uint64).reshape(-1, 2)
    return c, np.array(flags, np.uint8), np.array(wo, np.uint64)


def unitig_strings(g):
    return [g.sequence(u) for u in range(len(g.out[2]))]


def brute_segments(reads, k, seqs):
    """-> [(read, start, length, u, q, d)] by the rule over strings, and the number of windows found in some unitig string"""
    where = {}
    for u, s in enumerate(seqs):
        for q, w in enumerate(_kmers_of(s, k)):
            for key in (w, _rc(w)):
                assert where.setdefault(key, (u, q)) == (u, q), "a k-mer in two places"
    out, found = [], 0
    for r, read in enumerate(reads):
        prev = None
        for t, w in enumerate(_kmers_of(read, k) if len(read) >= k else []):
            if w not in where:
                prev = None
                continue
            found += 1
            u, q = where[w]
            d = 1 if w == _rc(w) or w != seqs[u][q:q + k] else 0
            if prev is not None and prev[0] == u and prev[2] == d and q == prev[1] + (1 if d == 0 else -1):
                out[-1][2] += 1
            else:
                out.append([r, t, 1, u, q, d])
            prev = (u, q, d)
    return [tuple(s) for s in out], found


def decode(path_offsets, segments):
    """the records as (read, start, length, u, q, d) tuples; checks the offsets against the read column"""
    recs = [(int(a), int(b) & 0xFFFFFFFF, int(b) >> 32, int(c), int(e) >> 1, int(e) & 1) for a, b, c, e in segments.tolist()]
    for r in range(len(path_offsets) - 1):
        assert all(rec[0] == r for rec in recs[int(path_offsets[r]):int(path_offsets[r + 1])])
    assert int(path_offsets[0]) == 0 and int(path_offsets[-1]) == len(recs)
    assert recs == sorted(recs, key=lambda s: (s[0], s[1]))
    return recs


def check(reads, g):
    """the reference's records of `reads` over the unitigs of g: right, maximal and covering, by strings alone"""
    k = g.k
    seqs = unitig_strings(g)
    canon, flags, wo = windows_of(reads, k)
    place = path_np.place_np(g.out[0], g.out[1], len(g.nodes))
    recs = decode(*path_np.read_paths_np(canon, flags, wo, g.tk, place, g.out[1]))
    covered = set()
    for r, start, length, u, q, d in recs:
        piece = reads[r][start:start + length + k - 1]
        assert len(piece) == length + k - 1 and length >= 1
        if d == 0:
            assert piece == seqs[u][q:q + length + k - 1], (r, start, length, u, q, d)
        else:
            assert q - length + 1 >= 0 and piece == _rc(seqs[u][q - length + 1:q + k]), (r, start, length, u, q, d)
        for t in range(start, start + length):
            assert (r, t) not in covered
            covered.add((r, t))
    want, found = brute_segments(reads, k, seqs)
    assert recs == want                        # maximal runs, and only the breaks the rule asks for
    assert len(covered) == found               # every window some unitig string holds is covered exactly once
    return recs, seqs


def _mutate(rng, s, p):
    return s[:p] + LETTERS[(LETTERS.index(s[p]) + 1 + int(rng.integers(0, 3))) % 4] + s[p + 1:]


def _reads_over(rng, genome, k, n=30):
    """reads tiled over a sequence: forward and reverse-complemented, one base substituted, an N, shorter than k, empty"""
    reads = []
    for i in range(n):
        a = int(rng.integers(0, max(len(genome) - 3 * k, 1)))
        read = genome[a:a + int(rng.integers(k, 4 * k + 1))]
        if i % 2:
            read = _rc(read)
        if i % 5 == 0:
            read = _mutate(rng, read, len(read) // 2)
        if i % 7 == 0:
            read = read[:len(read) // 3] + "N" + read[len(read) // 3 + 1:]
        reads.append(read)
    return reads + [genome, _rc(genome), genome[:k - 1], "", genome[:k]]


@pytest.mark.parametrize("k", KS)
def test_branching_graph(k):
    rng = np.random.default_rng(5400 + k)
    genome = _random_seq(rng, 40 * k)
    variant = _mutate(rng, genome, len(genome) // 2)                    # a bubble
    g = Graph(_kmers_of(genome, k) + _kmers_of(variant, k), k)
    assert len(g.out[2]) >= 4
    recs, seqs = check(_reads_over(rng, genome, k) + [variant], g)
    per_read = {}
    for rec in recs:
        per_read.setdefault(rec[0], []).append(rec)
    assert any(len(v) >= 3 for v in per_read.values())                  # a read across junctions
    assert any(rec[5] == 1 for rec in recs) and any(rec[5] == 0 for rec in recs)
    assert any(rec[4] > 0 and rec[5] == 0 for rec in recs)              # a read that enters a unitig inside it


@pytest.mark.parametrize("k", KS)
def test_hairpin(k):
    """a read that walks a unitig and then its mirror: the direction changes, the unitig does not"""
    if k in HAIRPINS:
        hp = HAIRPINS[k]
    else:
        stem = _random_seq(np.random.default_rng(5500 + k), 2 * k)
        hp = stem + _rc(stem)
    g = Graph(_kmers_of(hp, k), k)
    recs, seqs = check([hp, _rc(hp), hp[:len(hp) // 2], hp[1:-1]], g)
    first = [rec for rec in recs if rec[0] == 0]
    assert len(first) >= 2 and {rec[5] for rec in first} == {0, 1}
    if k % 2 == 0:                                                        # the palindrome in the middle: a segment of its own, d = 1
        pal = [rec for rec in first if rec[2] == 1 and seqs[rec[3]] == _rc(seqs[rec[3]])]
        assert len(pal) == 1 and pal[0][5] == 1 and pal[0][4] == 0


@pytest.mark.parametrize("k", KS)
def test_circle_with_a_read_of_more_than_two_laps(k):
    rng = np.random.default_rng(5600 + k)
    m = 3 * k + 7
    for _ in range(200):                                                  # (at small k a random circle may repeat a (k - 1)-mer: draw again)
        circle = _random_seq(rng, m)
        g = Graph(_kmers_of(circle + circle[:k - 1], k), k)
        if len(g.out[2]) == 1 and int(g.out[2][0]) == 1 and int(g.out[1][1]) == m:
            break
    assert len(g.out[2]) == 1 and int(g.out[2][0]) == 1 and int(g.out[1][1]) == m
    laps = (circle * 4)[3:3 + 2 * m + m // 2 + k - 1]                    # 2.5 laps, from base 3
    recs, seqs = check([laps, _rc(laps), circle], g)
    fw = [rec for rec in recs if rec[0] == 0]
    assert len(fw) in (3, 4) and sum(rec[2] for rec in fw) == 2 * m + m // 2
    assert all(rec[4] == (0 if rec[5] == 0 else m - 1) for rec in fw[1:])   # every passage starts at the written start (the mirror: at the end)
    assert any(rec[2] == m for rec in fw)                                # a whole lap is one segment


@pytest.mark.parametrize("k", KS)
def test_singletons_left_out(k):
    """min_count = 2: the k-mers seen once are in no unitig and their windows are unmapped"""
    rng = np.random.default_rng(5700 + k)
    genome = _random_seq(rng, 30 * k)
    once = _random_seq(rng, 6 * k)
    g = Graph(_kmers_of(genome, k) * 2 + _kmers_of(once, k), k, min_count=2)
    assert not all(g.present) and any(g.present)
    place = path_np.place_np(g.out[0], g.out[1], len(g.nodes))
    assert [bool(x) for x in place] == g.present
    reads = _reads_over(rng, genome, k) + [once, genome[:3 * k] + once[:3 * k]]
    recs, _ = check(reads, g)
    canon, flags, wo = windows_of(reads, k)
    unmapped = path_np.window_places_np(canon, flags, g.tk, place)[int(wo[-3]):int(wo[-2])] == 0
    assert unmapped.tolist() == [not g.present[g.index[min(w, _rc(w), key=_val)]] for w in _kmers_of(once, k)] and unmapped.sum() > k


def test_place_np_marks_first_and_last():
    nodes = np.array([2 * 4 + 1, 2 * 0, 2 * 9, 2 * 2 + 1, 2 * 7], np.uint64)     # unitigs (4', 0, 9), (2'), (7); entry 9 is beyond n
    offsets = np.array([0, 3, 4, 5], np.uint64)
    place = path_np.place_np(nodes, offsets, 8)
    assert place.tolist() == [(2 << 3), 0, (4 << 3) | 6 | 1, 0, (1 << 3) | 2 | 1, 0, 0, (5 << 3) | 6]
    assert path_np.place_np(nodes[:0], offsets[:1], 3).tolist() == [0, 0, 0]


def test_no_table_or_no_unitigs_gives_no_segments():
    canon, flags, wo = windows_of(["ACGTACGT", "", "AC"], 5)
    for tk, place, offsets in ((np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(1, np.uint64)),
                               (np.unique(canon), np.zeros(len(np.unique(canon)), np.uint64), np.zeros(1, np.uint64))):
        po, segs = path_np.read_paths_np(canon, flags, wo, tk, place, offsets)
        assert po.tolist() == [0, 0, 0, 0] and segs.shape == (0, 4)
