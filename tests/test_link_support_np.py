"""The host reference of the link support and the cut (tests/link_support_np.py), pinned on the CPU against Python strings.

The support of a link is, by strings alone, the number of times the reads spell the (k + 1)-mer the link spells -- the last k bases
of t followed by base k - 1 of t' -- on either strand, a (k + 1)-mer that is its own reverse complement once per occurrence.  That
count never sees a segment, a position or a slot.  At even k a link into a palindromic k-mer may lack its mirror slot, so there the
reference is compared with the rule written a second time over decoded tuples instead.  The cut is pinned by what it must leave:
nothing cut is the edges; everything cut keeps every unitig's entries together and leaves no link.  No GPU, no oracle, no library."""
import collections

import numpy as np
import pytest

from tests import link_np, link_support_np, path_np, unitig_np
from tests.test_link_np import links_of, oriented_sequences
from tests.test_path_np import _reads_over, decode, windows_of
from tests.test_unitig_np import HAIRPINS, LETTERS, Graph, _kmers_of, _random_seq, _rc, _strings_for


def _mutate(rng, s, p):
    return s[:p] + LETTERS[(LETTERS.index(s[p]) + 1 + int(rng.integers(0, 3))) % 4] + s[p + 1:]


def arrays_of(g, reads, min_count=1):
    """-> (edges, flips, nbr, place, link_offsets, targets, path_offsets, segments) of the reference chain"""
    e, f, nb, place, lo, tg = links_of(g, min_count)
    canon, flags, wo = windows_of(reads, g.k)
    po, segs = path_np.read_paths_np(canon, flags, wo, g.tk, place, g.out[1])
    return e, f, nb, place, lo, tg, po, segs


def spelled(g, lo, tg):
    """the (k + 1)-mer of every link slot"""
    seqs = oriented_sequences(g)
    return [seqs[t][-g.k:] + seqs[t2][g.k - 1] for t, t2 in link_np.link_pairs(lo, tg)]


def occurrences(reads, k, mers):
    seen = collections.Counter(w for read in reads for w in _kmers_of(read, k + 1) if all(ch in LETTERS for ch in w))
    return [seen[m] + (seen[_rc(m)] if _rc(m) != m else 0) for m in mers]


def check_against_strings(g, reads, min_count=1):
    e, f, nb, place, lo, tg, po, segs = arrays_of(g, reads, min_count)
    support, summary = link_support_np.link_support_np(segs, g.out[1], lo, tg)
    assert support.tolist() == occurrences(reads, g.k, spelled(g, lo, tg))
    junctions, crossed, unlinked = (int(x) for x in summary)
    assert unlinked == 0 and junctions == crossed
    pairs = link_np.link_pairs(lo, tg)
    hairpins = sum(int(support[x]) for x, (t, t2) in enumerate(pairs) if t2 == t ^ 1)
    assert int(support.sum()) == 2 * crossed - hairpins          # a crossing credits the link and its mirror; a hairpin is both
    again, summary2 = link_support_np.link_support_np(segs, g.out[1], lo, tg, support, summary)
    assert again.tolist() == (2 * support).tolist() and summary2.tolist() == (2 * summary).tolist()   # accumulated into
    return support, pairs, (e, f, nb, place, lo, tg, po, segs)


def rule_support(recs, sizes, pairs, n_links):
    """the rule of include/kmx.h once more, over decoded tuples and the list of (t, t') pairs"""
    first = {}
    for x, pair in enumerate(pairs):
        first.setdefault(pair, x)
    support, crossed, unlinked = [0] * n_links, 0, []
    for (r, start, length, u, q, d), (r2, start2, _, u2, q2, d2) in zip(recs[:-1], recs[1:]):
        if r != r2 or start2 != start + length:
            continue
        at_exit = q + length - 1 == sizes[u] - 1 if d == 0 else q - (length - 1) == 0
        at_entry = q2 == 0 if d2 == 0 else q2 == sizes[u2] - 1
        t, t2 = 2 * u + d, 2 * u2 + d2
        if not (at_exit and at_entry and (t, t2) in first):
            unlinked.append((u, u2))
            continue
        crossed += 1
        for x in {first[(t, t2)], first.get((t2 ^ 1, t ^ 1))} - {None}:
            support[x] += 1
    return support, [crossed + len(unlinked), crossed, len(unlinked)], unlinked


@pytest.mark.parametrize("k", (5, 9))
def test_bubble_graph(k):
    rng = np.random.default_rng(5400 + k)
    genome = _random_seq(rng, 40 * k)
    variant = _mutate(rng, genome, len(genome) // 2)
    g = Graph(_kmers_of(genome, k) + _kmers_of(variant, k), k)
    assert len(g.out[2]) >= 4
    support, pairs, _ = check_against_strings(g, _reads_over(rng, genome, k) + [variant], 1)
    assert (support > 1).any()
    by_pair = dict(zip(pairs, support.tolist()))
    assert all(by_pair[(b ^ 1, a ^ 1)] == s for (a, b), s in by_pair.items())   # a link and its mirror carry the same number


@pytest.mark.parametrize("k", (5, 9))
def test_kmers_no_read_spans_have_support_zero(k):
    """the variant's k-mers are in the table but only the genome is read: the two links into the variant's branch stay at 0"""
    rng = np.random.default_rng(5400 + k)
    genome = _random_seq(rng, 40 * k)
    variant = _mutate(rng, genome, len(genome) // 2)
    g = Graph(_kmers_of(genome, k) + _kmers_of(variant, k), k)
    support, pairs, _ = check_against_strings(g, [genome, _rc(genome), genome[k:5 * k]], 1)
    assert (support == 0).any() and (support > 0).any()
    # min_count = 2: the k-mers seen once are in no unitig; a read over them is unmapped there and crosses nothing
    once = _random_seq(rng, 6 * k)
    g = Graph(_kmers_of(genome, k) * 2 + _kmers_of(once, k), k, min_count=2)
    check_against_strings(g, [genome, once, genome[:3 * k] + once[:3 * k]], 2)


@pytest.mark.parametrize("k", (5, 9))
def test_hairpin_counts_once(k):
    rng = np.random.default_rng(5450 + k)
    for _ in range(200):
        stem = _random_seq(rng, 3 * k)
        g = Graph(_kmers_of(stem + _rc(stem), k), k)
        if len(g.out[2]) == 1:
            break
    assert len(g.out[2]) == 1
    hp = stem + _rc(stem)
    support, pairs, _ = check_against_strings(g, [hp, hp, _rc(hp), hp[k:-k], stem], 1)
    assert len(pairs) == 1 and pairs[0][1] == pairs[0][0] ^ 1
    assert support.tolist() == [4]                                  # hp reads the same on both strands: once per read that crosses


@pytest.mark.parametrize("k", (5, 9))
def test_circle_with_a_read_of_more_than_two_laps(k):
    rng = np.random.default_rng(5600 + k)
    m = 3 * k + 7
    for _ in range(200):
        circle = _random_seq(rng, m)
        g = Graph(_kmers_of(circle + circle[:k - 1], k), k)
        if len(g.out[2]) == 1 and int(g.out[2][0]) == 1 and int(g.out[1][1]) == m:
            break
    assert len(g.out[2]) == 1 and int(g.out[2][0]) == 1
    laps = (circle * 4)[3:3 + 2 * m + m // 2 + k - 1]
    support, pairs, _ = check_against_strings(g, [laps, _rc(laps), circle], 1)
    assert pairs == [(0, 0), (1, 1)]
    # the written start lies anywhere on the circle: the laps pass it two or three times on each strand, the single lap at most once
    assert support[0] == support[1] and 4 <= int(support[0]) <= 7


@pytest.mark.parametrize("k", (6, 8))
def test_even_k_follows_the_rule_as_written(k):
    rng = np.random.default_rng(5800 + k)
    for strings in (_strings_for(k, rng), _kmers_of(HAIRPINS[k], k)):
        g = Graph(strings, k)
        words = [g.sequence(u) for u in range(len(g.out[2]))]
        reads = [HAIRPINS[k], _rc(HAIRPINS[k])] + [w for w in words if len(w) > k][:40]
        walk = words[0]                                             # a read that follows links from unitig to unitig
        e, f, nb, place, lo, tg = links_of(g)
        seqs, t = oriented_sequences(g), 0
        for _ in range(60):
            nxt = tg[int(lo[t]):int(lo[t + 1])]
            if len(nxt) == 0:
                break
            t = int(nxt[int(rng.integers(0, len(nxt)))])
            walk += seqs[t][k - 1:]
        reads += [walk, _rc(walk), walk[3:len(walk) // 2]]
        e, f, nb, place, lo, tg, po, segs = arrays_of(g, reads)
        support, summary = link_support_np.link_support_np(segs, g.out[1], lo, tg)
        sizes = np.diff(g.out[1].astype(np.int64)).tolist()
        want, want_summary, unlinked = rule_support(decode(po, segs), sizes, link_np.link_pairs(lo, tg), len(tg))
        assert support.tolist() == want and summary.tolist() == want_summary
        assert int(summary[1]) > 0
        # a palindromic window always reads d = 1, a link into the palindrome names the orientation of the node it comes from: the
        # two may differ, and only such a junction finds no slot
        pal = {u for u, w in enumerate(words) if w == _rc(w)}
        assert all(u in pal or u2 in pal for u, u2 in unlinked)
        # what still holds by strings at even k: a slot never holds more than its (k + 1)-mer occurs
        assert all(s <= o for s, o in zip(want, occurrences(reads, k, spelled(g, lo, tg))))


def test_garbage_gives_the_defined_result():
    """unitig indices beyond U, targets beyond 2 U, offsets that do not ascend: every junction is counted, none outside the lists"""
    rng = np.random.default_rng(5900)
    n_unitigs, n_links = 6, 9
    offsets = np.array([0, 4, 3, 9, 9, 12, 20], np.uint64)
    lo = rng.integers(0, n_links + 3, 2 * n_unitigs + 1).astype(np.uint64)
    tg = rng.integers(0, 2 * n_unitigs + 4, n_links).astype(np.uint64)
    segs = np.zeros((300, 4), np.uint64)
    segs[:, 0] = np.sort(rng.integers(0, 4, 300))
    segs[:, 2] = rng.integers(0, n_unitigs + 2, 300)
    segs[:, 3] = rng.integers(0, 12, 300)
    start = 0
    for s in range(300):
        length = int(rng.integers(0, 4))
        segs[s, 1] = (length << 32) | start
        start = (start + length + int(rng.integers(0, 5) == 0)) % 2**32
    support, summary = link_support_np.link_support_np(segs, offsets, lo, tg)
    assert int(summary[0]) == int(summary[1]) + int(summary[2]) > 100 and int(summary[2]) > 0
    assert int(support.sum()) <= 2 * int(summary[1])


@pytest.mark.parametrize("k", (5, 9))
def test_cut_nothing_and_cut_everything(k):
    rng = np.random.default_rng(5400 + k)
    genome = _random_seq(rng, 40 * k)
    variant = _mutate(rng, genome, len(genome) // 2)
    circle = _random_seq(rng, 3 * k + 7)
    g = Graph(_kmers_of(genome, k) + _kmers_of(variant, k) + _kmers_of(circle + circle[:k - 1], k), k)
    n = len(g.nodes)
    e, f, nb, place, lo, tg = links_of(g)
    cut = lambda mask: link_support_np.adjacency_cut_np(e, f, nb, n, g.out[0], g.out[1], place, lo, mask)
    assert cut(np.zeros(len(tg), np.uint8)).tolist() == e.tolist()
    out = cut(np.ones(len(tg), np.uint8))
    assert (out & ~e).max() == 0 and sum(bin(int(a ^ b)).count("1") for a, b in zip(e, out)) == len(tg)   # one bit per slot
    nodes2, offsets2, circular2, _ = unitig_np.unitigs_np(g.tk, g.tc, k, 1, out, f, nb)
    entries = lambda nodes, offs: {frozenset(int(v) >> 1 for v in nodes[int(a):int(b)]) for a, b in zip(offs[:-1], offs[1:])}
    assert entries(nodes2, offsets2) == entries(g.out[0], g.out[1])      # as sets: a circle becomes linear
    assert not circular2.any()
    place2 = path_np.place_np(nodes2, offsets2, n)
    lo2, tg2 = link_np.links_of_unitigs_np(out, f, nb, n, nodes2, offsets2, place2)
    assert len(tg2) == 0 and not lo2.any()
    # one slot cut: its bit alone; its mirror's slot cut as well: the edge is gone in both directions and the rest is as it was
    pairs = link_np.link_pairs(lo, tg)
    x = next(x for x, (a, b) in enumerate(pairs) if a >> 1 != b >> 1)
    mask = np.zeros(len(tg), np.uint8)
    mask[x] = 1
    assert sum(bin(int(a ^ b)).count("1") for a, b in zip(e, cut(mask))) == 1
    mask[pairs.index((pairs[x][1] ^ 1, pairs[x][0] ^ 1))] = 1
    out = cut(mask)
    nodes3, offsets3, _, _ = unitig_np.unitigs_np(g.tk, g.tc, k, 1, out, f, nb)
    lo3, tg3 = link_np.links_of_unitigs_np(out, f, nb, n, nodes3, offsets3, path_np.place_np(nodes3, offsets3, n))
    assert len(offsets3) <= len(g.out[1]) and len(tg3) <= len(tg) - 2


@pytest.mark.parametrize("k", (5, 9))
def test_pruning_keeps_every_crossing(k):
    """support 0 cut, unitigs rebuilt, reads threaded again: nothing is unlinked, every link left is walked, and the crossings that
    are gone are exactly the pairs of segments that the rebuilt unitigs join into one"""
    rng = np.random.default_rng(6000 + k)
    genome = _random_seq(rng, 40 * k)
    variant = _mutate(rng, genome, len(genome) // 2)
    g = Graph(_kmers_of(genome, k) + _kmers_of(variant, k), k)
    n = len(g.nodes)
    reads = _reads_over(rng, genome, k)
    support, pairs, (e, f, nb, place, lo, tg, po, segs) = check_against_strings(g, reads, 1)
    mask = link_support_np.unsupported_np(support)
    assert mask.any() and not mask.all()
    out = link_support_np.adjacency_cut_np(e, f, nb, n, g.out[0], g.out[1], place, lo, mask)
    nodes2, offsets2, _, _ = unitig_np.unitigs_np(g.tk, g.tc, k, 1, out, f, nb)
    place2 = path_np.place_np(nodes2, offsets2, n)
    lo2, tg2 = link_np.links_of_unitigs_np(out, f, nb, n, nodes2, offsets2, place2)
    canon, flags, wo = windows_of(reads, k)
    po2, segs2 = path_np.read_paths_np(canon, flags, wo, g.tk, place2, offsets2)
    support2, summary2 = link_support_np.link_support_np(segs2, offsets2, lo2, tg2)
    _, summary = link_support_np.link_support_np(segs, g.out[1], lo, tg)
    assert int(summary2[2]) == 0 and (support2 >= 1).all()
    assert len(offsets2) <= len(g.out[1])
    assert int(summary[1]) - int(summary2[1]) == len(segs) - len(segs2)


def _compositions():
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("bench_link_support", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                                                                       "bench_link_support.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("k", (5, 9))
def test_bench_compositions_equal_the_reference(k):
    """the torch compositions that tools/bench_link_support.py races the calls against, on the CPU"""
    import torch

    mod = _compositions()
    rng = np.random.default_rng(6100 + k)
    genome = _random_seq(rng, 40 * k)
    variant = _mutate(rng, genome, len(genome) // 2)
    g = Graph(_kmers_of(genome, k) + _kmers_of(variant, k), k)
    reads = _reads_over(rng, genome, k)
    support, pairs, (e, f, nb, place, lo, tg, po, segs) = check_against_strings(g, reads, 1)
    _, summary = link_support_np.link_support_np(segs, g.out[1], lo, tg)
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64))
    got, got_summary = mod.support_composition(i64(segs).reshape(-1, 4), i64(g.out[1]), i64(lo), i64(tg))
    assert got.numpy().view(np.uint64).tolist() == support.tolist() and got_summary.tolist() == summary.tolist()
    for mask in (link_support_np.unsupported_np(support), np.ones(len(tg), np.uint8), np.zeros(len(tg), np.uint8)):
        want = link_support_np.adjacency_cut_np(e, f, nb, len(g.nodes), g.out[0], g.out[1], place, lo, mask)
        out = mod.cut_composition(torch.from_numpy(e), torch.from_numpy(f), i64(nb).reshape(-1), i64(place), i64(g.out[0]), i64(g.out[1]), i64(lo),
                                  torch.from_numpy(mask))
        assert out.numpy().tolist() == want.tolist()
