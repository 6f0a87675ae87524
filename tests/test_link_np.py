"""The host reference of the unitig links and the selection (tests/link_np.py), pinned on the CPU against brute force over Python
strings, and with it the host-side pieces that need no device: Unitigs.tips, Unitigs.write_gfa and the torch compositions of
tools/bench_unitig_links.py.

The brute force never sees an index, an edge byte or a place.  It spells the unitigs (tests/unitig_np.sequences_np); the sequence
of the oriented unitig 2 u + 1 is the reverse complement of that of u; and t -> t' iff the last k - 1 bases of seq(t) are the first
k - 1 bases of seq(t').  A palindromic one-node unitig spells the same in both orientations: the brute force sees both 2 u' and
2 u' + 1 where the rule picks one, so the orientation bit of such a unitig is cleared on both ends before anything is compared;
everything else is compared exactly.  No GPU, no oracle, no library."""
import io

import numpy as np
import pytest
import torch

from tests import link_np
from tests.test_unitig_np import HAIRPINS, Graph, _kmers_of, _random_seq, _rc, _strings_for

CIRCLE_KS = (15, 31, 33, 47)


def _mutate(rng, s, p):
    return s[:p] + "ACGT"[("ACGT".index(s[p]) + 1 + int(rng.integers(0, 3))) % 4] + s[p + 1:]


def oriented_sequences(g):
    seqs = [g.sequence(u) for u in range(len(g.out[2]))]
    return [s if t & 1 == 0 else _rc(s) for s in seqs for t in (0, 1)]


def brute_links(g):
    """-> {t: set of t'} by overlap of k - 1 bases over the unitig strings"""
    k, seqs = g.k, oriented_sequences(g)
    starts = {}
    for t, s in enumerate(seqs):
        starts.setdefault(s[:k - 1], []).append(t)
    return {t: set(starts.get(s[len(s) - (k - 1):], ())) for t, s in enumerate(seqs)}


def links_of(g, min_count=1):
    e, f, nb = link_np.graph_np.adjacency_np(g.tk, g.tc, g.k, min_count)
    place = link_np.place_np(g.out[0], g.out[1], len(g.nodes))
    return (e, f, nb, place) + link_np.links_of_unitigs_np(e, f, nb, len(g.nodes), g.out[0], g.out[1], place)


def check(g, min_count=1):
    """the reference's links of g: the brute force's, in ascending c, mirror-symmetric; returns (pairs, palindromic unitigs)"""
    seqs = oriented_sequences(g)
    pal = {t >> 1 for t, s in enumerate(seqs) if s == _rc(s)}
    assert all(len(seqs[2 * u]) == g.k for u in pal)                        # only a one-node unitig spells a palindrome
    norm = lambda t: t & ~1 if t >> 1 in pal else t
    e, f, nb, place, lo, tg = links_of(g, min_count)
    assert len(lo) == 2 * len(g.out[2]) + 1 and int(lo[0]) == 0 and int(lo[-1]) == len(tg)
    pairs = link_np.link_pairs(lo, tg)
    assert len(set(pairs)) == len(pairs)                                    # no link twice
    want = brute_links(g)
    for t in range(len(seqs)):
        mine = [b for a, b in pairs if a == t]
        assert len(mine) <= 4
        assert {norm(b) for b in mine} == {norm(b) for b in want[t]}, (g.k, t, mine, want[t])
        if not any(b >> 1 in pal for b in mine):
            assert set(mine) == want[t]                                     # exactly, where no palindrome is involved
        # ascending c: the base that follows the overlap in the target's spelling -- c itself out of an exit node read forward, its
        # complement out of one read in reverse (a predecessor P_c of the key is the successor that appends comp(c) to its mirror)
        a, b = int(g.out[1][t >> 1]), int(g.out[1][(t >> 1) + 1])
        o = (int(g.out[0][b - 1]) if t & 1 == 0 else int(g.out[0][a]) ^ 1) & 1
        nxt = ["ACGT".index(seqs[b2][g.k - 1]) for b2 in mine]
        assert nxt == sorted(nxt, reverse=bool(o)), (g.k, t, nxt)
    # mirror symmetry: exact without palindromic unitigs, modulo their orientation with them
    if not pal:
        link_np.assert_mirror_symmetric(lo, tg)
    folded = {(norm(a), norm(b)) for a, b in pairs}
    assert folded == {(norm(b ^ 1), norm(a ^ 1)) for a, b in pairs}
    for u in pal:                                                           # the two orientations of a palindrome: the same neighbours
        assert sorted(norm(b) for a, b in pairs if a == 2 * u) == sorted(norm(b) for a, b in pairs if a == 2 * u + 1)
    return pairs, pal


@pytest.mark.parametrize("min_count", (1, 2))
@pytest.mark.parametrize("k", (4, 5, 6, 8))
def test_dense_tables(k, min_count):
    rng = np.random.default_rng(5100 + k)
    g = Graph(_strings_for(k, rng), k, min_count)
    pairs, pal = check(g, min_count)
    lo = links_of(g, min_count)[4]
    deg = np.diff(lo.astype(np.int64))
    assert deg.max() == 4 if k <= 5 else (deg == 0).any() and (deg >= 2).any()   # sides with four links; dead ends and forks
    if k == 5:
        assert any(a == b ^ 1 for a, b in pairs)                            # hairpins: a unitig that runs into its own mirror
    if k % 2 == 0:
        assert pal and any(b >> 1 in pal for _, b in pairs)                 # links into palindromes
    assert any(a == b for a, b in pairs)                                    # a self-link (a circle, or the all-A k-mer)
    if min_count == 2:
        assert not all(g.present)


@pytest.mark.parametrize("k", (5, 6, 9))
def test_bubble(k):
    rng = np.random.default_rng(5400 + k)
    genome = _random_seq(rng, 40 * k)
    variant = _mutate(rng, genome, len(genome) // 2)
    g = Graph(_kmers_of(genome, k) + _kmers_of(variant, k), k)
    assert len(g.out[2]) >= 4
    pairs, _ = check(g)
    deg = np.diff(links_of(g)[4].astype(np.int64))
    assert (deg >= 2).any() and (deg == 1).any() and ((deg == 0).any() or k == 5)   # (at k = 5 the ends of 200 random bases branch too)


@pytest.mark.parametrize("k", (6, 8))
def test_hairpins(k):
    g = Graph(_kmers_of(HAIRPINS[k], k), k)
    pairs, pal = check(g)
    assert len(pal) == 1 and len(g.out[2]) == 2
    (p,) = pal
    # the stem runs into the palindrome, in the orientation of the node it leaves, and comes back out of it as its own mirror
    (a, b), = [(a, b) for a, b in pairs if a >> 1 != p]
    first, last = int(g.out[0][int(g.out[1][a >> 1])]), int(g.out[0][int(g.out[1][(a >> 1) + 1]) - 1])
    assert b == 2 * p + ((last if a & 1 == 0 else first ^ 1) & 1)
    assert sorted(pairs) == sorted([(a, b), (2 * p, a ^ 1), (2 * p + 1, a ^ 1)])


@pytest.mark.parametrize("k", (5, 9))
def test_odd_hairpin_links_to_its_mirror(k):
    """a stem and its reverse complement at odd k: no palindromic k-mer, one unitig whose exit overlaps the entry of its mirror"""
    rng = np.random.default_rng(5450 + k)
    for _ in range(200):
        stem = _random_seq(rng, 3 * k)
        g = Graph(_kmers_of(stem + _rc(stem), k), k)
        if len(g.out[2]) == 1:
            break
    assert len(g.out[2]) == 1 and not g.out[2][0]
    pairs, pal = check(g)
    assert not pal and len(pairs) == 1 and pairs[0][1] == pairs[0][0] ^ 1


@pytest.mark.parametrize("k", CIRCLE_KS)
def test_a_circle_links_to_itself(k):
    rng = np.random.default_rng(5200 + k)
    circle = _random_seq(rng, k + 40)
    g = Graph(_kmers_of(circle + circle[:k - 1], k), k)
    assert len(g.out[2]) == 1 and int(g.out[2][0]) == 1
    pairs, _ = check(g)
    assert pairs == [(0, 0), (1, 1)]


@pytest.mark.parametrize("k", (4, 15, 33))
def test_all_a_links_to_itself(k):
    g = Graph(["A" * k], k)
    pairs, _ = check(g)
    assert pairs == [(0, 0), (1, 1)]


def test_inconsistent_inputs_stay_inside():
    """any bytes in edges / flips / nbr / place over valid unitigs: a result, every target below 2 U"""
    rng = np.random.default_rng(5460)
    g = Graph(_kmers_of(_random_seq(rng, 400), 9), 9)
    n, n_unitigs = len(g.nodes), len(g.out[2])
    edges, flips = rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 256, n).astype(np.uint8)
    nbr = rng.integers(0, n + 50, (n, 8)).astype(np.uint64)
    place = rng.integers(0, 8 * (n + 5), n).astype(np.uint64)
    lo, tg = link_np.links_of_unitigs_np(edges, flips, nbr, n, g.out[0], g.out[1], place)
    assert len(tg) > 0 and (tg < 2 * n_unitigs).all() and (np.diff(lo.astype(np.int64)) <= 4).all()
    assert link_np.links_of_unitigs_np(edges[:0], flips[:0], nbr[:0], 0, g.out[0][:0], g.out[1][:1], place[:0])[0].tolist() == [0]


def test_select_np():
    rng = np.random.default_rng(5470)
    genome, once = _random_seq(rng, 300), _random_seq(rng, 60)
    g = Graph(_kmers_of(genome, 9) * 2 + _kmers_of(_mutate(rng, genome, 150), 9) * 2 + _kmers_of(once, 9), 9, min_count=2)
    n_unitigs = len(g.out[2])
    assert n_unitigs >= 4 and not all(g.present)
    place = link_np.place_np(g.out[0], g.out[1], len(g.nodes))
    keep = np.zeros(n_unitigs, np.uint8)
    keep[::2] = 1
    sk, sc = link_np.select_np(g.tk, g.tc, place, g.out[1], keep)
    kept = sorted(int(v) >> 1 for u in range(0, n_unitigs, 2) for v in g.out[0][int(g.out[1][u]):int(g.out[1][u + 1])])
    assert sk.tolist() == g.tk[kept].tolist() and sc.tolist() == g.tc[kept].tolist()
    ak, ac = link_np.select_np(g.tk, g.tc, place, g.out[1], np.ones(n_unitigs, np.uint8))
    assert ak.tolist() == g.tk[np.array(g.present)].tolist()                # all ones: the present entries
    assert len(link_np.select_np(g.tk, g.tc, place, g.out[1], np.zeros(n_unitigs, np.uint8))[0]) == 0


# ---------------------------------------------------------------- tips and GFA on a hand-written graph
# k = 5.  MAIN forks after ...TTGTA: MAIN goes on with G, the TIP with T for three more bases (three nodes, a dead end); RING is a
# circle of eight nodes, ISLE a stretch of two nodes that touches nothing.  No 4-mer occurs twice on either strand.
K = 5
MAIN = "ATTGGGCTTGTAGTCACCCCTC"
TIP = "TGTATCT"
RING = "AACACGGG"
ISLE = "TCGGTT"


def _hand_graph():
    from kmers_amd.api import UnitigLinks, Unitigs

    g = Graph(_kmers_of(MAIN, K) + _kmers_of(TIP, K) + _kmers_of(RING + RING[:K - 1], K) + _kmers_of(ISLE, K), K)
    e, f, nb, place, lo, tg = links_of(g)
    check(g)
    t = lambda a, dt=np.int64: torch.from_numpy(np.asarray(a).astype(dt))
    un = Unitigs(t(g.out[0]), t(g.out[1]), t(g.out[2], np.uint8), t(g.out[3]), len(g.out[2]), K, None, None, t(g.seq, np.uint8))
    return g, un, UnitigLinks(t(lo), t(tg))


def _which(g, s):
    """the unitig that spells s or its reverse complement"""
    (u,) = [u for u in range(len(g.out[2])) if g.sequence(u) in (s, _rc(s))]
    return u


def test_tips_on_a_hand_written_graph():
    g, un, links = _hand_graph()
    assert un.n_unitigs == 5
    left, right, tip = _which(g, MAIN[:12]), _which(g, MAIN[8:]), _which(g, TIP)
    ring = [u for u in range(5) if g.out[2][u]][0]
    isle = _which(g, ISLE)
    assert len({left, right, tip, ring, isle}) == 5
    assert un.lengths.tolist()[tip] == 3 and un.lengths.tolist()[isle] == 2 and un.lengths.tolist()[ring] == 8
    assert sorted(links.degrees[left].tolist()) == [0, 2] and sorted(links.degrees[right].tolist()) == [0, 1]
    assert links.degrees[ring].tolist() == [1, 1] and links.degrees[isle].tolist() == [0, 0]
    assert links.sources().tolist() == [a for a, _ in link_np.link_pairs(links.offsets.numpy(), links.targets.numpy())]
    mask = lambda *us: [u in us for u in range(5)]
    assert un.tips(links, 3).tolist() == mask(tip)
    assert un.tips(links, 2).tolist() == mask()
    assert un.tips(links, 3, islands=True).tolist() == mask(tip, isle)
    assert un.tips(links, 100).tolist() == mask(left, right, tip)           # both branches of the fork are dead ends: both go
    assert un.tips(links, 100, islands=True).tolist() == mask(left, right, tip, isle)   # never the circle


def test_gfa_of_a_hand_written_graph():
    g, un, links = _hand_graph()
    out = io.StringIO()
    un.write_gfa(out, links)
    lines = out.getvalue().splitlines()
    assert lines[0] == "H\tVN:Z:1.0"
    seg = {}
    for ln in lines[1:6]:
        tag, name, s, ln_tag, kc = ln.split("\t")
        assert tag == "S" and ln_tag == f"LN:i:{len(s)}" and kc == f"KC:i:{int(g.out[3][int(name)])}"
        assert s == g.sequence(int(name))
        seg[name] = s
    assert sorted(seg) == ["0", "1", "2", "3", "4"]
    got = set()
    for ln in lines[6:]:
        tag, a, sa, b, sb, ov = ln.split("\t")
        assert tag == "L" and ov == "4M"
        x = seg[a] if sa == "+" else _rc(seg[a])
        y = seg[b] if sb == "+" else _rc(seg[b])
        assert x[-4:] == y[:4]
        got.add((a, sa, b, sb))
    assert len(got) == len(lines) - 6 == 3                                  # left -> right, left -> tip, the ring onto itself
    pairs = link_np.link_pairs(links.offsets.numpy(), links.targets.numpy())
    want = {min((a, b), (b ^ 1, a ^ 1)) for a, b in pairs}
    assert got == {(str(a >> 1), "+-"[a & 1], str(b >> 1), "+-"[b & 1]) for a, b in want}
    assert len(want) == (len(pairs) + sum(1 for a, b in pairs if (b ^ 1, a ^ 1) == (a, b))) // 2
    plain = io.StringIO()
    un.write_gfa(plain)
    assert plain.getvalue().splitlines() == lines[:6]                       # without links: the header and the segments


# ---------------------------------------------------------------- the bench tool's torch compositions
def _compositions():
    from tools import bench_unitig_links

    return bench_unitig_links.links_composition, bench_unitig_links.select_composition


@pytest.mark.parametrize("k,min_count", ((4, 1), (6, 2), (8, 1), (33, 1)))
def test_bench_compositions_equal_the_reference(k, min_count):
    links_composition, select_composition = _compositions()
    rng = np.random.default_rng(5100 + k)
    g = Graph(_strings_for(k, rng), k, min_count)
    e, f, nb, place, lo, tg = links_of(g, min_count)
    t = lambda a: torch.from_numpy(np.asarray(a).view(np.int64) if np.asarray(a).dtype == np.uint64 else np.asarray(a))
    glo, gtg = links_composition(t(e), t(f), t(nb), t(place), t(g.out[0]), t(g.out[1]))
    assert glo.tolist() == lo.tolist() and gtg.tolist() == tg.tolist()
    keep = (rng.random(len(g.out[2])) < 0.5).astype(np.uint8)
    counts = g.tc if g.tc is not None else np.ones(len(g.nodes), np.uint64)
    sk, sc = link_np.select_np(g.tk, counts, place, g.out[1], keep)
    gk, gc = select_composition(t(g.tk), t(counts), t(place), t(g.out[1]), t(keep))
    assert np.array_equal(gk.numpy().view(np.uint64), sk) and np.array_equal(gc.numpy().view(np.uint64), sc)


def test_bench_links_composition_on_inconsistent_inputs():
    links_composition, _ = _compositions()
    rng = np.random.default_rng(5480)
    g = Graph(_kmers_of(_random_seq(rng, 400), 9), 9)
    n = len(g.nodes)
    edges, flips = rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 256, n).astype(np.uint8)
    nbr = rng.integers(0, n + 50, (n, 8)).astype(np.uint64)
    nbr[::7, 3] = np.uint64(2**64 - 1)
    place = rng.integers(0, 8 * (n + 5), n).astype(np.uint64)
    lo, tg = link_np.links_of_unitigs_np(edges, flips, nbr, n, g.out[0], g.out[1], place)
    t = lambda a: torch.from_numpy(np.asarray(a).view(np.int64) if np.asarray(a).dtype == np.uint64 else np.asarray(a))
    glo, gtg = links_composition(t(edges), t(flips), t(nbr), t(place), t(g.out[0]), t(g.out[1]))
    assert glo.tolist() == lo.tolist() and gtg.tolist() == tg.tolist()
