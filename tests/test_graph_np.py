"""The host reference of the graph layer (tests/graph_np.py), pinned on the CPU against brute force over Python strings.

The brute force knows k-mers as strings over ACGT (codes 0..3, complement 3 - c, base i at bits [2i, 2i + 1]): a successor of s is
s[1:] + c, a predecessor c + s[:-1], the reverse complement is the reversed string complemented, and the node of a word is whichever of
the word and its reverse complement has the smaller VALUE (a Python int, so the last base weighs most).  Nodes live in a dict.  None
of it shifts, masks or looks anything up in a sorted array, so it cannot share a mistake with the numpy code.
No GPU, no oracle, no library."""
import numpy as np
import pytest

from tests import graph_np

LETTERS = "ACGT"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
KS = [2, 3, 4, 5, 6, 31, 33, 34, 64]


# ---------------------------------------------------------------- brute force
def _val(s):
    return sum(LETTERS.index(ch) << (2 * i) for i, ch in enumerate(s))


def _rc(s):
    return "".join(COMP[ch] for ch in reversed(s))


def _canon(s):
    r = _rc(s)
    return r if _val(r) < _val(s) else s


def _table(strings, k, counts=None):
    """canonical strings -> (sorted node strings, keys in the table's layout, counts)"""
    nodes = sorted({_canon(s) for s in strings}, key=_val)
    vals = [_val(s) for s in nodes]
    if k <= 31:
        tk = np.array(vals, np.uint64).reshape(-1)
    else:
        tk = np.array([[v & (2**64 - 1), v >> 64] for v in vals], np.uint64).reshape(-1, 2)
    return nodes, tk, counts


def _brute_adjacency(nodes, counts, min_count):
    index = {s: i for i, s in enumerate(nodes)}
    present = [counts is None or int(counts[i]) >= min_count for i in range(len(nodes))]
    edges, flips, nbr = [], [], []
    for i, s in enumerate(nodes):
        eb = fb = 0
        row = [2**64 - 1] * 8
        for e in range(8):
            c = LETTERS[e & 3]
            w = s[1:] + c if e < 4 else c + s[:-1]
            node = _canon(w)
            j = index.get(node)
            if not present[i] or j is None or not present[j]:
                continue
            eb |= 1 << e
            if _val(_rc(w)) < _val(w):
                fb |= 1 << e
            row[e] = j
        edges.append(eb)
        flips.append(fb)
        nbr.append(row)
    return np.array(edges, np.uint8), np.array(flips, np.uint8), np.array(nbr, np.uint64).reshape(-1, 8)


def _kmers_of(seq, k):
    return [seq[i:i + k] for i in range(len(seq) - k + 1)]


def _random_seq(rng, n):
    return "".join(LETTERS[c] for c in rng.integers(0, 4, n))


def _strings_for(k, rng):
    """a few hundred k-mers at most: small k -- a random half of all words, so degrees reach 4 and palindromes occur; large k -- the
    k-mers of overlapping stretches of one sequence with substitutions, so paths, forks and tips occur; always the all-A word"""
    if k <= 6:
        words = ["".join(LETTERS[(v >> (2 * i)) & 3] for i in range(k)) for v in range(4**k)]
        keep = rng.random(len(words)) < (0.8 if k <= 3 else 0.5 if k <= 5 else 0.08)
        out = [w for w, kp in zip(words, keep) if kp]
    else:
        base = _random_seq(rng, k + 90)
        out = _kmers_of(base, k)
        for _ in range(3):
            at = int(rng.integers(0, len(base) - k - 20))
            piece = list(base[at:at + k + 20])
            p = int(rng.integers(1, len(piece) - 1))
            piece[p] = LETTERS[(LETTERS.index(piece[p]) + 1) & 3]
            out += _kmers_of("".join(piece), k)
    if k % 2 == 0:   # a palindrome and its neighbours
        half = _random_seq(rng, k // 2)
        pal = half + _rc(half)
        assert pal == _rc(pal)
        out += [pal, pal[1:] + "A", "C" + pal[:-1], pal[1:] + "G"]
    return out + ["A" * k]


# ---------------------------------------------------------------- adjacency
@pytest.mark.parametrize("k", KS)
def test_adjacency_matches_the_strings(k):
    rng = np.random.default_rng(1000 + k)
    nodes, tk, _ = _table(_strings_for(k, rng), k)
    n = len(nodes)
    assert 1 < n <= 600
    tc = rng.integers(1, 4, n).astype(np.uint64)
    some_edge = False
    for counts, mc in ((None, 1), (tc, 1), (tc, 2), (tc, 4)):
        want = _brute_adjacency(nodes, counts, mc)
        got = graph_np.adjacency_np(tk, counts, k, mc)
        for w, g, name in zip(want, got, ("edges", "flips", "nbr")):
            assert np.array_equal(w, g), (k, mc, name)
        some_edge |= bool(want[0].any())
        if counts is not None and mc == 4:
            assert not want[0].any()   # above every count: nobody is present
    assert some_edge
    edges, flips, _ = graph_np.adjacency_np(tk, None, k)
    assert (flips & ~edges).max() == 0   # bits of absent edges are 0
    assert flips.any() and (edges & ~flips).any()   # both strands occur


@pytest.mark.parametrize("k", [4, 6, 34, 64])
def test_palindromic_neighbour_is_not_flipped(k):
    rng = np.random.default_rng(7 + k)
    half = _random_seq(rng, k // 2)
    pal = half + _rc(half)
    before, after = "C" + pal[:-1], pal[1:] + "G"
    nodes, tk, _ = _table([pal, before, after], k)
    edges, flips, nbr = graph_np.adjacency_np(tk, None, k)
    ip = nodes.index(pal)
    for s in (before, after):
        i = nodes.index(_canon(s))
        hits = [e for e in range(8) if int(nbr[i, e]) == ip]
        assert hits, s
        for e in hits:
            assert (int(edges[i]) >> e) & 1 and not (int(flips[i]) >> e) & 1
    want = _brute_adjacency(nodes, None, 1)
    assert np.array_equal(want[0], edges) and np.array_equal(want[1], flips) and np.array_equal(want[2], nbr)


@pytest.mark.parametrize("k", KS)
def test_all_a_is_its_own_successor_and_predecessor(k):
    nodes, tk, _ = _table(["A" * k], k)
    edges, flips, nbr = graph_np.adjacency_np(tk, None, k)
    assert edges.tolist() == [0x11] and flips.tolist() == [0]
    assert [int(v) for v in nbr[0]] == [0, 2**64 - 1, 2**64 - 1, 2**64 - 1, 0, 2**64 - 1, 2**64 - 1, 2**64 - 1]
    assert graph_np.unitig_ends_np(edges, flips, nbr).tolist() == [3]   # its one neighbour is itself: both sides end


@pytest.mark.parametrize("k", KS)
def test_every_edge_has_its_reverse(k):
    """an edge i -> j in slot e: j lists i on the side the edge enters (unflipped successor edge: the predecessor side, and so on), in
    the slot of the base i loses there, flipped like the edge itself -- unless i is a palindrome, whose word is never flipped"""
    rng = np.random.default_rng(2000 + k)
    nodes, tk, _ = _table(_strings_for(k, rng), k)
    edges, flips, nbr = graph_np.adjacency_np(tk, None, k)
    n_edges = 0
    for i, s in enumerate(nodes):
        first, last = LETTERS.index(s[0]), LETTERS.index(s[-1])
        for e in range(8):
            if not (int(edges[i]) >> e) & 1:
                continue
            n_edges += 1
            j, f = int(nbr[i, e]), (int(flips[i]) >> e) & 1
            if e < 4:   # i loses its first base
                back = 4 + first if not f else 3 - first
            else:       # i loses its last base
                back = last if not f else 4 + (3 - last)
            assert int(nbr[j, back]) == i, (s, e, nodes[j], back)
            assert (int(edges[j]) >> back) & 1
            assert (int(flips[j]) >> back) & 1 == (f if s != _rc(s) else 0)
    assert n_edges > 0


# ---------------------------------------------------------------- unitig ends and the histogram
def _distinct_path(rng, k, n_bases):
    """a sequence whose k-mers are distinct nodes and whose (k-1)-mers are distinct too: a non-branching path"""
    for _ in range(100):
        s = _random_seq(rng, n_bases)
        km = [_canon(w) for w in _kmers_of(s, k)]
        k1 = [_canon(w) for w in _kmers_of(s, k - 1)]
        if len(set(km)) == len(km) and len(set(k1)) == len(k1):
            return s
    raise AssertionError("no such sequence")


def _ends_of(strings, k):
    nodes, tk, _ = _table(strings, k)
    edges, flips, nbr = graph_np.adjacency_np(tk, None, k)
    want = _brute_adjacency(nodes, None, 1)
    assert np.array_equal(want[0], edges) and np.array_equal(want[2], nbr)
    return nodes, edges, graph_np.unitig_ends_np(edges, flips, nbr)


def _bits(ends):
    return int((ends & 1).sum() + ((ends >> 1) & 1).sum())


@pytest.mark.parametrize("k", [11, 33])
def test_unitigs_of_hand_made_graphs(k):
    """2 * unitigs = set end bits: a path is one unitig, a fork three, a path with a tip three, a cycle none (it has no end)"""
    rng = np.random.default_rng(31 + k)
    path = _distinct_path(rng, k, k + 40)
    nodes, edges, ends = _ends_of(_kmers_of(path, k), k)
    assert _bits(ends) == 2 and sorted(bin(int(b)).count("1") for b in edges).count(1) == 2
    # only the path's two outer nodes end anything
    outer = {_canon(path[:k]), _canon(path[-k:])}
    assert {nodes[i] for i in np.nonzero(ends)[0]} == outer

    # a fork: two continuations of the same stem
    stem = path[:k + 15]
    other = stem + LETTERS[(LETTERS.index(path[k + 15]) + 1) & 3] + _distinct_path(rng, k, k + 10)
    _, edges, ends = _ends_of(_kmers_of(path, k) + _kmers_of(other, k), k)
    assert _bits(ends) == 6
    assert sum(1 for b in edges.tolist() if bin(b & 15).count("1") == 2 or bin(b >> 4).count("1") == 2) == 1

    # a tip: the same, the second continuation two k-mers long
    tip = stem + LETTERS[(LETTERS.index(path[k + 15]) + 2) & 3] + "A"
    _, edges, ends = _ends_of(_kmers_of(path, k) + _kmers_of(tip, k), k)
    assert _bits(ends) == 6

    # a cycle: the sequence closed on itself
    ring = _distinct_path(rng, k, k + 25)
    _, edges, ends = _ends_of(_kmers_of(ring + ring[:k - 1], k), k)
    assert all(bin(b & 15).count("1") == 1 and bin(b >> 4).count("1") == 1 for b in edges.tolist())
    assert _bits(ends) == 0

    # an isolated node is a unitig of its own
    _, edges, ends = _ends_of([path[:k]], k)
    assert edges.tolist() == [0] and ends.tolist() == [3]


def test_unitig_ends_ignores_indices_outside_the_table():
    edges = np.array([0x11, 0x11], np.uint8)
    flips = np.zeros(2, np.uint8)
    nbr = np.full((2, 8), graph_np.NO_ENTRY, np.uint64)
    nbr[0, 0], nbr[0, 4] = 1, 7          # slot 4 names an entry that does not exist
    nbr[1, 4], nbr[1, 0] = 0, 2**40
    assert graph_np.unitig_ends_np(edges, flips, nbr).tolist() == [2, 1]


def test_edge_histogram_and_summary():
    rng = np.random.default_rng(5)
    edges = rng.integers(0, 256, 5000).astype(np.uint8)
    edges[:700] = 0x11
    edges[700:900] = 0
    hist = graph_np.edge_hist_np(edges)
    assert hist.dtype == np.uint64 and len(hist) == 256 and int(hist.sum()) == 5000
    for b in (0, 0x11, 0xFF, 37):
        assert int(hist[b]) == edges.tolist().count(b)
    s = graph_np.graph_summary_np(hist)
    assert s["n_edges"] == sum(bin(b).count("1") for b in edges.tolist())
    assert s["n_isolated"] == int(hist[0]) and s["n_interior"] == int(s["degrees"][1, 1])
    assert int(s["degrees"].sum()) == 5000 and int(s["degrees"][0, 0]) == s["n_isolated"]
    assert s["n_tips"] == int(s["degrees"][0, 1:].sum() + s["degrees"][1:, 0].sum())
    assert graph_np.edge_hist_np(np.zeros(0, np.uint8)).tolist() == [0] * 256
