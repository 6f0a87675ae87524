"""The host reference of the component rule (tests/component_np.py), pinned on the CPU: against graphs written out by hand, against a
second implementation (a breadth-first search over the explicit edge set, and scipy's connected_components where scipy imports),
and on the identities the rule implies.  With it the pieces that need no device: UnitigComponents.keep and mean_counts on host
tensors, the synchronous model of the device's schedule on the three long chains (the round counts DESIGN 4.6.12 quotes, under the
cap the device test asserts), and Context.count_drop_small_components on the host.  No GPU, no oracle, no library."""
import math

import numpy as np
import pytest
import torch

from tests import clean_np, component_np
from tests.component_np import NONE, both_ways, components_np, link_arrays

CHAIN = 1 << 16


def round_cap(U):
    """what the device test allows a doubling schedule: it needs about log2 U jumps after the first hook, a walk needs about U"""
    return 8 * math.ceil(math.log2(U)) + 16


def chain_pairs(order):
    """a chain through the unitigs in the given order"""
    return [(int(a), int(b)) for a, b in zip(order[:-1], order[1:])]


def chain_orders(U=CHAIN):
    return {"index order": np.arange(U), "reverse order": np.arange(U)[::-1], "permuted": np.random.default_rng(1234).permutation(U)}


def lists_to_arrays(lists):
    lo = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    return lo, np.array([t for l in lists for t in l], np.uint64)


# ---------------------------------------------------------------- graphs written out by hand
def test_two_chains_and_an_isolated_unitig():
    # 0 - 2 - 4, 1 - 3 - 6, 5 alone; lengths 1 .. 7, sums 10 u
    lo, tg = link_arrays(7, both_ways([(0, 2), (2, 4), (1, 3), (3, 6)]))
    offsets = np.concatenate([[0], np.cumsum(np.arange(1, 8))]).astype(np.uint64)
    sums = (10 * np.arange(7)).astype(np.uint64)
    labels, ids, rec, C = components_np(offsets, sums, lo, tg)
    assert labels.tolist() == [0, 1, 0, 1, 0, 5, 1] and ids.tolist() == [0, 1, 0, 1, 0, 2, 1] and C == 3
    assert rec.tolist() == [[0, 3, 1 + 3 + 5, 0 + 20 + 40], [1, 3, 2 + 4 + 7, 10 + 30 + 60], [5, 1, 6, 50]]
    assert components_np(None, None, lo, tg)[2].tolist() == [[0, 3, 3, 3], [1, 3, 3, 3], [5, 1, 1, 1]]   # m = 1, S = m
    assert components_np(offsets, None, lo, tg)[2].tolist() == [[0, 3, 9, 9], [1, 3, 13, 13], [5, 1, 6, 6]]


def test_a_link_in_one_direction_only():
    lo, tg = link_arrays(4, [(3, 1), (0, 2)])
    assert components_np(None, None, lo, tg)[0].tolist() == [0, 1, 0, 1]


def test_self_link_and_hairpin_join_nothing():
    # 0 -> 0 (a circular unitig), 1 -> mirror(1) (a hairpin), 2 -> mirror(2) and 2 -> 3
    lo, tg = lists_to_arrays([[0], [1], [3], [], [5, 6], [], [], [4]])
    labels, ids, rec, C = components_np(None, None, lo, tg)
    assert labels.tolist() == [0, 1, 2, 2] and C == 3 and rec[:, 1].tolist() == [1, 1, 2]


def test_a_masked_bridge_splits_a_component():
    lo, tg = link_arrays(5, both_ways([(0, 1), (1, 2), (2, 3), (3, 4)]))
    assert components_np(None, None, lo, tg)[3] == 1
    labels, ids, rec, C = components_np(None, None, lo, tg, mask=np.array([1, 1, 0, 7, 1], np.uint8))
    assert labels.tolist() == [0, 0, NONE, 3, 3] and ids.tolist() == [0, 0, NONE, 1, 1] and C == 2
    assert rec.tolist() == [[0, 2, 2, 2], [3, 2, 2, 2]]                      # the bridge is counted nowhere
    assert components_np(None, None, lo, tg, mask=np.zeros(5, np.uint8))[3] == 0


def test_garbage_lists_are_empty():
    U = 4
    # side 0 of unitig 0: descending offsets; side 1 of 0: a target >= 2 U next to a good one; side 0 of 1: five links; side 1 of 1: fine
    lo = np.array([5, 3, 5, 10, 11, 11, 11, 11, 2**63], np.uint64)
    tg = np.array([2, 2, 2, 4, 8, 6, 6, 6, 6, 6, 4], np.uint64)
    lists = component_np.valid_lists(lo, tg, U)
    assert lists == [[], [], [], [4], [], [], [], []]
    assert components_np(None, None, lo, tg)[0].tolist() == [0, 1, 1, 3]
    lo[3], lo[4] = 12, 12                                                    # hi beyond n_links: nothing is left
    assert components_np(None, None, lo, tg)[3] == 4
    lo = np.array([0, 4, 4, 4, 4], np.uint64)                                # one bad target empties the whole list
    assert components_np(None, None, lo, np.array([2, 2, 4, 2], np.uint64))[0].tolist() == [0, 1]
    assert components_np(None, None, lo, np.array([2, 2, 2, 2], np.uint64))[0].tolist() == [0, 0]
    offsets = np.array([7, 3, 10], np.uint64)                                # descending unitig offsets: m = 0
    assert components_np(offsets, None, lo, np.array([2, 2, 2, 2], np.uint64))[2].tolist() == [[0, 2, 7, 7]]


# ---------------------------------------------------------------- a second implementation
def bfs_labels(pairs, alive):
    U = len(alive)
    nb = [[] for _ in range(U)]
    for u, v in pairs:
        nb[u].append(v)
        nb[v].append(u)
    labels = [NONE] * U
    for s in range(U):                                                       # ascending: the first unitig to reach a component is its minimum
        if alive[s] and labels[s] == NONE:
            labels[s], todo = s, [s]
            while todo:
                for v in nb[todo.pop()]:
                    if labels[v] == NONE:
                        labels[v] = s
                        todo.append(v)
    return labels


def random_graph(rng, U, links_per_unitig, garbage=0.0):
    """sparse random links, each listed in one direction only (a unitig's sides fill up: no more than eight)"""
    deg = np.zeros(U, np.int64)
    directed = []
    for u, v in rng.integers(0, U, (int(links_per_unitig * U), 2)).tolist():
        if deg[u] < 8:
            deg[u] += 1
            directed.append((u, v))
    lo, tg = link_arrays(U, directed)
    if garbage:
        wild = rng.random(len(lo)) < garbage
        lo[wild] = rng.integers(0, len(tg) + 6, int(wild.sum())).astype(np.uint64)
        wild = rng.random(len(tg)) < garbage
        tg[wild] = rng.integers(0, 2 * U + 3, int(wild.sum())).astype(np.uint64)
    return lo, tg


@pytest.mark.parametrize("garbage", (0.0, 0.05))
@pytest.mark.parametrize("U", (1, 2, 50, 3000))
def test_against_bfs_and_scipy(U, garbage):
    rng = np.random.default_rng(4100 + U)
    for links, masked in ((0.6, False), (1.5, True), (0.0, False)):
        lo, tg = random_graph(rng, U, links, garbage)
        mask = (rng.random(U) < 0.8).astype(np.uint8) * 3 if masked else None
        offsets = np.concatenate([[0], np.cumsum(rng.integers(1, 30, U))]).astype(np.uint64)
        sums = rng.integers(0, 2**64, U, dtype=np.uint64)
        labels, ids, rec, C = components_np(offsets, sums, lo, tg, mask)
        pairs, alive = component_np.edges_np(lo, tg, U, mask)
        assert labels.tolist() == bfs_labels(pairs, alive)
        live = np.array(alive)
        # the identities: fixed points, the minimum, ids ascending with the roots, the sums
        lab = labels[live].astype(np.int64)
        assert (labels[lab] == labels[live]).all() and (lab <= np.nonzero(live)[0]).all()
        assert (labels[~live] == NONE).all() and (ids[~live] == NONE).all()
        assert rec[:, 0].tolist() == sorted(set(lab.tolist())) and C == len(rec)
        assert (rec[ids[live].astype(np.int64), 0] == labels[live]).all()
        m = np.diff(offsets.astype(np.int64))
        assert int(rec[:, 1].sum()) == int(live.sum()) and int(rec[:, 2].sum()) == int(m[live].sum())
        assert int(rec[:, 3].sum(dtype=np.uint64)) == int(sums[live].sum(dtype=np.uint64))
        # the model of the device's schedule gives the same labels
        assert component_np.rounds_model(lo, tg, U, mask)[0] == labels.tolist()
        try:
            from scipy.sparse import coo_matrix
            from scipy.sparse.csgraph import connected_components
        except ImportError:
            continue
        e = np.array(sorted(pairs), np.int64).reshape(-1, 2)
        n_sc, lab_sc = connected_components(coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(U, U)), directed=False)
        assert len(set(lab_sc[live].tolist())) == C
        first = {}
        for u in np.nonzero(live)[0].tolist():
            first.setdefault(int(lab_sc[u]), u)
        assert [first[int(c)] for c in lab_sc[live]] == lab.tolist()


# ---------------------------------------------------------------- the schedule's synchronous model on the long chains
@pytest.mark.parametrize("name", ("index order", "reverse order", "permuted"))
def test_rounds_of_the_model_on_a_long_chain(name):
    """hook + one jump per round, every launch reading the state it began with: 17 rounds in index and in reverse order, 15 on
    the permuted chain, for 2^16 unitigs -- doubling, not a walk of the chain; the cap is the device test's"""
    order = chain_orders()[name]
    lo, tg = link_arrays(CHAIN, both_ways(chain_pairs(order)))
    labels, rounds = component_np.rounds_model(lo, tg, CHAIN)
    assert set(labels) == {0}
    assert rounds <= round_cap(CHAIN), rounds
    assert rounds == {"index order": 17, "reverse order": 17, "permuted": 15}[name]


# ---------------------------------------------------------------- the torch composition of tools/bench_unitig_components.py
@pytest.mark.parametrize("masked", (False, True))
def test_bench_composition_equals_the_reference(masked):
    import importlib.util
    import os

    from kmers_amd.api import UnitigLinks, Unitigs

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bench_unitig_components.py")
    spec = importlib.util.spec_from_file_location("bench_unitig_components", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(4300)
    U = 2000
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64))
    for links_per_unitig in (0.0, 0.6, 1.2):
        lo, tg = random_graph(rng, U, links_per_unitig)
        offsets = np.concatenate([[0], np.cumsum(rng.integers(1, 30, U))]).astype(np.uint64)
        sums = rng.integers(0, 2**64, U, dtype=np.uint64)
        mask = (rng.random(U) < 0.8) if masked else None
        want = components_np(offsets, sums, lo, tg, None if mask is None else mask.astype(np.uint8))
        un = Unitigs(None, t(offsets), None, t(sums), U, 31)
        labels, ids, rec, rounds = tool.components_composition(un, UnitigLinks(t(lo), t(tg)), None if mask is None else torch.from_numpy(mask))
        assert np.array_equal(labels.numpy().view(np.uint64), want[0]) and np.array_equal(ids.numpy().view(np.uint64), want[1])
        assert np.array_equal(rec.numpy().view(np.uint64), want[2]) and rounds >= 1


# ---------------------------------------------------------------- UnitigComponents on host tensors
def _components(labels, ids, rec, C):
    from kmers_amd.api import UnitigComponents

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64))
    return UnitigComponents(t(labels), t(ids), t(rec).view(-1, 4), C, 0)


def test_keep_and_mean_counts():
    # components of 3, 3, 1, 2 unitigs; nodes 9, 13, 6, 13: two of equal size
    lo, tg = link_arrays(9, both_ways([(0, 2), (2, 4), (1, 3), (3, 6), (7, 8)]))
    offsets = np.array([0, 1, 3, 6, 10, 15, 21, 28, 30, 41], np.uint64)
    sums = np.array([5, 5, 5, 5, 5, 2**63, 5, 2**63, 2**63 + 4], np.uint64)
    mask = np.array([1, 1, 1, 1, 1, 1, 1, 1, 1], np.uint8)
    labels, ids, rec, C = components_np(offsets, sums, lo, tg, mask)
    assert rec[:, 2].tolist() == [9, 13, 6, 13] and rec[:, 3].tolist() == [15, 15, 2**63, 4]
    comp = _components(labels, ids, rec, C)
    assert comp.roots.tolist() == [0, 1, 5, 7] and comp.n_unitigs.tolist() == [3, 3, 1, 2] and comp.n_nodes.tolist() == [9, 13, 6, 13]
    assert comp.mean_counts.tolist() == [15 / 9, 15 / 13, 2.0**63 / 6, 4 / 13]
    for kw in (dict(), dict(min_nodes=7), dict(min_nodes=13), dict(min_unitigs=3), dict(min_count_sum=15), dict(min_count_sum=16),
               dict(min_count_sum=2**63), dict(min_count_sum=2**63 + 1), dict(min_nodes=7, min_unitigs=3, min_count_sum=5),
               dict(largest=0), dict(largest=1), dict(largest=2), dict(largest=3), dict(largest=9), dict(largest=2, min_unitigs=3)):
        got = comp.keep(**kw)
        assert got.dtype == torch.uint8 and got.tolist() == component_np.keep_np(ids, rec, **kw).tolist(), kw
    assert comp.keep(largest=1).tolist() == [0, 1, 0, 1, 0, 0, 1, 0, 0]      # 13 nodes twice: the smaller id
    assert comp.keep(largest=2).tolist() == [0, 1, 0, 1, 0, 0, 1, 1, 1]
    assert comp.keep(min_count_sum=2**63).tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0]
    # a unitig the mask left out is kept by nothing
    mask[2] = 0
    labels, ids, rec, C = components_np(offsets, sums, lo, tg, mask)
    comp = _components(labels, ids, rec, C)
    assert C == 5 and comp.keep().tolist() == [1, 1, 0, 1, 1, 1, 1, 1, 1]
    assert comp.keep().tolist() == component_np.keep_np(ids, rec).tolist()
    none = _components(*components_np(offsets, sums, lo, tg, np.zeros(9, np.uint8)))
    assert none.keep().tolist() == [0] * 9 and none.roots.numel() == 0


def test_read_paths_components_is_a_gather():
    from kmers_amd.api import ReadPaths

    lo, tg = link_arrays(4, both_ways([(0, 2)]))
    comp = _components(*components_np(None, None, lo, tg, np.array([1, 0, 1, 1], np.uint8)))
    seg = torch.tensor([[0, 0, 2, 0], [0, 0, 3, 0], [1, 0, 1, 0], [2, 0, 0, 0]], dtype=torch.int64)
    assert ReadPaths(torch.tensor([0, 2, 3, 4]), seg, 5).components(comp).tolist() == [0, 1, -1, 0]


# ---------------------------------------------------------------- a small component that every cleaning rule keeps
def fork_cases(k):
    """a backbone and, from a second sequence, a fork of three unitigs: a stem and two branches, each longer than every limit of the
    cleaning rule's defaults and equally covered -> [(sequence, times)], the backbone, the three pieces"""
    from tests.test_clean_np import COMP, _random_seq

    rng = np.random.default_rng(8800 + k)
    main = _random_seq(rng, 500)
    stem, a, b = _random_seq(rng, 3 * k), _random_seq(rng, 3 * k), _random_seq(rng, 3 * k)
    if a[0] == b[0]:
        b = COMP[b[0]] + b[1:]
    return [(main, 6), (stem + a, 3), (stem[-(k - 1):] + b, 3)], main, (stem, a, b)


@pytest.mark.parametrize("k", (15, 31))
def test_drop_small_components_on_the_host(k):
    from tests.test_clean_np import key_list, table

    seqs, main, _ = fork_cases(k)
    tk, tc = table(seqs, k)
    sk, sc, log = clean_np.simplify_np(tk, tc, k, **clean_np.rule_of(k, island_max_nodes=k))
    assert np.array_equal(sk, tk) and log[0]["removed"] == 0                 # no rule of the cleaning call touches the fork
    gk, gc, (labels, ids, rec, C) = component_np.drop_small_np(tk, tc, k, min_nodes=len(main) - k + 1)
    assert C == 2 and sorted(rec[:, 1].tolist()) == [1, 3]                   # the backbone, and a component of three unitigs
    wk, wc = table([(main, 6)], k)
    assert key_list(gk) == key_list(wk) and np.array_equal(gc, wc)
    assert np.array_equal(component_np.drop_small_np(tk, tc, k, min_nodes=1)[0], tk)
