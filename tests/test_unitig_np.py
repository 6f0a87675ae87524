"""The host reference of the unitig layer (tests/unitig_np.py), pinned on the CPU against brute force over Python strings.

The brute force knows k-mers as strings over ACGT (codes 0..3, base i at bits [2i, 2i + 1], so the last base weighs most), nodes as a
sorted list of canonical strings, and a link as string overlap: the oriented word w of a node goes on to the one present word
w[1:] + c if that word's only present predecessor is w, the two are different entries and neither is its own reverse complement.
It shifts nothing, masks nothing and never sees an edge byte.  No GPU, no oracle, no library."""
import numpy as np
import pytest

from tests import graph_np, unitig_np

LETTERS = "ACGT"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
KS = [4, 5, 6, 8, 15, 31, 33, 47]
HAIRPINS = {6: "GGTTACGTAACC", 8: "CCAGTACGTACTGG"}


def _val(s):
    return sum(LETTERS.index(ch) << (2 * i) for i, ch in enumerate(s))


def _rc(s):
    return "".join(COMP[ch] for ch in reversed(s))


def _canon(s):
    r = _rc(s)
    return r if _val(r) < _val(s) else s


def _kmers_of(seq, k):
    return [seq[i:i + k] for i in range(len(seq) - k + 1)]


def _random_seq(rng, n):
    return "".join(LETTERS[c] for c in rng.integers(0, 4, n))


class Graph:
    """a table from strings (with how often each canonical string occurred), its reference unitigs and the brute-force links"""

    def __init__(self, strings, k, min_count=1, with_counts=True):
        self.k = k
        occ = {}
        for s in strings:
            occ[_canon(s)] = occ.get(_canon(s), 0) + 1
        self.nodes = sorted(occ, key=_val)
        vals = [_val(s) for s in self.nodes]
        self.tk = (np.array(vals, np.uint64).reshape(-1) if k <= 31
                   else np.array([[v & (2**64 - 1), v >> 64] for v in vals], np.uint64).reshape(-1, 2))
        self.tc = np.array([occ[s] for s in self.nodes], np.uint64) if with_counts else None
        self.index = {s: i for i, s in enumerate(self.nodes)}
        self.present = [self.tc is None or int(self.tc[i]) >= min_count for i in range(len(self.nodes))]
        e, f, nb = graph_np.adjacency_np(self.tk, self.tc, k, min_count)
        self.out = unitig_np.unitigs_np(self.tk, self.tc, k, min_count, e, f, nb)
        self.seq = unitig_np.sequences_np(self.tk, k, self.out[0], self.out[1])

    def word(self, v):
        s = self.nodes[v >> 1]
        return _rc(s) if v & 1 else s

    def _entry(self, w):
        i = self.index.get(_canon(w))
        return i if i is not None and self.present[i] else None

    def next(self, v):
        """brute force: the oriented node behind v, None if v has no link"""
        w = self.word(v)
        if not self.present[v >> 1] or w == _rc(w):
            return None
        succ = [w[1:] + c for c in LETTERS if self._entry(w[1:] + c) is not None]
        if len(succ) != 1:
            return None
        t = succ[0]
        j = self._entry(t)
        back = [c + t[:-1] for c in LETTERS if self._entry(c + t[:-1]) is not None]
        if len(back) != 1 or j == v >> 1 or t == _rc(t):
            return None
        return 2 * j + (0 if t == self.nodes[j] else 1)

    def unitigs(self):
        nodes, offsets, circular, sums = self.out
        return [([int(v) for v in nodes[int(offsets[u]):int(offsets[u + 1])]], int(circular[u]), int(sums[u])) for u in range(len(circular))]

    def sequence(self, u):
        at = int(self.out[1][u]) + u * (self.k - 1)
        return bytes(self.seq[at:at + int(self.out[1][u + 1] - self.out[1][u]) + self.k - 1]).decode()


def _check(g):
    """every property the definitions promise, against the brute-force links"""
    k, n = g.k, len(g.nodes)
    for v in range(2 * n):   # every link is mutual
        w = g.next(v)
        if w is not None:
            assert g.next(w ^ 1) == v ^ 1, (k, v, w)
    units = g.unitigs()
    where = {}
    for u, (vs, circ, total) in enumerate(units):
        entries = [v >> 1 for v in vs]
        assert len(set(entries)) == len(entries), (k, u, "an entry twice")
        for i in entries:
            assert i not in where and g.present[i], (k, u, i)
            where[i] = u
        for a, b in zip(vs, vs[1:]):
            assert g.next(a) == b, (k, u, a, b)
        if circ:
            assert g.next(vs[-1]) == vs[0], (k, u)
            assert vs[0] == 2 * min(entries), (k, u)                         # written from 2 i*
        else:
            assert g.next(vs[-1]) is None and g.next(vs[0] ^ 1) is None, (k, u)   # maximal: no link behind the tail or before the head
            assert entries[0] < entries[-1] or (len(vs) == 1 and vs[0] & 1 == 0), (k, u)
        s = g.sequence(u)
        assert len(s) == len(vs) + k - 1
        for t, v in enumerate(vs):
            assert s[t:t + k] == g.word(v), (k, u, t)                       # spells back to its keys, window by window
        assert total == (len(vs) if g.tc is None else sum(int(g.tc[i]) for i in entries) % 2**64)
    assert sorted(where) == [i for i in range(n) if g.present[i]]            # every present entry in exactly one unitig
    heads = [vs[0] >> 1 for vs, _, _ in units]
    assert heads == sorted(heads) and len(set(heads)) == len(heads)
    assert int(g.out[1][-1]) == len(g.out[0]) == len(where)
    return units


def _strings_for(k, rng):
    if k <= 6:
        words = ["".join(LETTERS[(v >> (2 * i)) & 3] for i in range(k)) for v in range(4**k)]
        keep = rng.random(len(words)) < (0.5 if k <= 5 else 0.08)
        strings = [w for w, kp in zip(words, keep) if kp]
        strings += _kmers_of(_random_seq(rng, 60), k) * 2
    else:
        genome = _random_seq(rng, 300)
        strings = []
        for _ in range(24):
            a = int(rng.integers(0, len(genome) - 80))
            read = list(genome[a:a + 80])
            for p in np.nonzero(rng.random(80) < 0.02)[0]:
                read[p] = LETTERS[int(rng.integers(0, 4))]
            strings += _kmers_of("".join(read), k)
        strings += _kmers_of(genome, k)
        circle = _random_seq(rng, k + 40)
        strings += _kmers_of(circle + circle[:k - 1], k) * 2
    strings.append("A" * k)
    strings += _kmers_of("AC" * 12, k) * 2 + _kmers_of("ACG" * 12, k) * 2
    if k in HAIRPINS:
        strings += _kmers_of(HAIRPINS[k], k) * 2
    return strings


@pytest.mark.parametrize("with_counts", (True, False))
@pytest.mark.parametrize("min_count", (1, 2))
@pytest.mark.parametrize("k", KS)
def test_reference_against_brute_force(k, min_count, with_counts):
    rng = np.random.default_rng(5100 + k)
    g = Graph(_strings_for(k, rng), k, min_count, with_counts)
    units = _check(g)
    if k >= 8:   # (in the dense graphs of small k nearly every node branches)
        assert any(c for _, c, _ in units)                 # the AC / ACG repeats and the circular sequence
        assert max(len(vs) for vs, _, _ in units) > 20
    if with_counts and min_count == 2:
        assert not all(g.present) and any(g.present)


@pytest.mark.parametrize("k", (6, 8))
def test_hairpins_are_two_unitigs(k):
    """y -> palindrome z -> rc(y): without the palindrome rule next would not be injective here"""
    g = Graph(_kmers_of(HAIRPINS[k], k), k)
    units = _check(g)
    pal = [i for i, s in enumerate(g.nodes) if s == _rc(s)]
    assert len(pal) == 1
    assert len(units) == 2 and sorted(len(vs) for vs, _, _ in units) == [1, len(g.nodes) - 1]
    assert [vs for vs, _, _ in units if len(vs) == 1] == [[2 * pal[0]]]
    assert not any(c for _, c, _ in units)


@pytest.mark.parametrize("k", (4, 15, 33))
def test_all_a_is_one_linear_node(k):
    g = Graph(["A" * k] * 3, k)
    assert _check(g) == [([0], 0, 3)]
    assert g.sequence(0) == "A" * k


def test_ac_repeat_is_a_circle_of_two():
    g = Graph(_kmers_of("AC" * 12, 5), 5)
    units = _check(g)
    assert len(units) == 1 and units[0][1] == 1 and len(units[0][0]) == 2
    assert g.sequence(0) in ("ACACAC", "CACACA", "GTGTGT", "TGTGTG")


@pytest.mark.parametrize("k", (15, 31, 33, 47))
def test_a_circular_sequence_is_one_circular_unitig(k):
    rng = np.random.default_rng(5200 + k)
    circle = _random_seq(rng, k + 40)
    g = Graph(_kmers_of(circle + circle[:k - 1], k), k)
    units = _check(g)
    assert len(units) == 1 and units[0][1] == 1 and len(units[0][0]) == k + 40
    s = g.sequence(0)
    assert len(s) == 2 * k + 39 and (s[:k + 40] in circle * 2 or s[:k + 40] in _rc(circle) * 2)   # a rotation of the circle, either strand


def test_garbage_inputs_still_give_disjoint_paths():
    """any bytes in edges / flips / nbr: the mutual links keep next injective, the walk ends and no entry is listed twice"""
    rng = np.random.default_rng(5300)
    n = 500
    edges, flips = rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 256, n).astype(np.uint8)
    nbr = rng.integers(0, n + 50, (n, 8)).astype(np.uint64)
    one = np.array([1 << e for e in rng.integers(0, 4, n)], np.uint8)
    edges[: n // 2] = one[: n // 2] | (one[::-1][: n // 2] << 4)   # many sides with one edge, so links do occur
    nodes, offsets, circular, sums = unitig_np.unitigs_np(None, None, 15, 1, edges, flips, nbr)
    assert sorted(int(v) >> 1 for v in nodes) == list(range(n))
    assert int(offsets[-1]) == n and (np.diff(offsets.astype(np.int64)) > 0).all()
    assert sums.tolist() == np.diff(offsets.astype(np.int64)).tolist()
