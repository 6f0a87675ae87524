"""Host reference of kmx_count_unitig_links and kmx_count_unitig_select(2), written straight from the definitions in include/kmx.h on
top of tests/graph_np.py (the adjacency), tests/unitig_np.py (the unitigs) and tests/path_np.place_np (the index): one loop over the
oriented unitigs that states the rule, one mask over the entries.  Nothing here knows about degree bytes, scans or slots.  Shared by
tests/test_gpu_unitig_links.py; pinned against brute force over Python strings in tests/test_link_np.py, which needs no GPU.

An oriented unitig is t = 2 * u + s (s = 1: the unitig read as its reverse complement); mirror(t) = t ^ 1."""
import numpy as np

from tests import graph_np, unitig_np
from tests.path_np import place_np


def links_of_unitigs_np(edges, flips, nbr, n, nodes, offsets, place):
    """-> (link_offsets uint64[2U + 1], targets uint64[L]): oriented unitig t owns targets[link_offsets[t]:link_offsets[t + 1]]"""
    edges, flips = np.asarray(edges, np.uint8), np.asarray(flips, np.uint8)
    nbr = np.asarray(nbr, np.uint64).reshape(-1, 8)
    offs = [int(x) for x in offsets]
    n_unitigs = len(offs) - 1
    n_nodes = offs[-1] if n_unitigs else 0
    link_offsets, targets = [0], []
    for t in range(2 * n_unitigs):
        a, b = offs[t >> 1], offs[(t >> 1) + 1]
        if a < b <= n_nodes:
            v = int(nodes[b - 1]) if t & 1 == 0 else int(nodes[a]) ^ 1          # the exit node
            i, o = v >> 1, v & 1
            for c in range(4) if i < n else ():
                e = 4 * o + c
                if not (int(edges[i]) >> e) & 1:
                    continue
                j = int(nbr[i, e])
                x = int(place[j]) if j < n else 0
                p = (x >> 3) - 1
                if x == 0 or p < 0 or p >= n_nodes:                             # no neighbour, in no unitig, outside the offsets
                    continue
                u2 = int(np.searchsorted(offsets, np.uint64(p), "right")) - 1
                w = o ^ ((int(flips[i]) >> e) & 1)                              # the orientation in which the neighbour is entered
                if w == x & 1 and x & 2:
                    targets.append(2 * u2)
                elif w != x & 1 and x & 4:
                    targets.append(2 * u2 + 1)
        link_offsets.append(len(targets))
    return np.array(link_offsets, np.uint64), np.array(targets, np.uint64)


def select_np(tk, tc, place, offsets, keep):
    """-> (keys, counts): the entries whose place is non-zero and whose unitig is kept, order kept"""
    tk, tc = np.asarray(tk, np.uint64), np.asarray(tc, np.uint64)
    n_unitigs = len(offsets) - 1
    n_nodes = int(offsets[-1]) if n_unitigs else 0
    mask = np.zeros(len(tc), bool)
    for i, x in enumerate(int(x) for x in place):
        p = (x >> 3) - 1
        if x != 0 and 0 <= p < n_nodes:
            mask[i] = keep[int(np.searchsorted(offsets, np.uint64(p), "right")) - 1] != 0
    return tk[mask], tc[mask]


def links_of_table_np(tk, tc, k, min_count=1):
    """a table -> (unitigs_np's four arrays, place, link_offsets, targets): the whole chain of references"""
    edges, flips, nbr = graph_np.adjacency_np(tk, tc, k, min_count)
    out = unitig_np.unitigs_np(tk, tc, k, min_count, edges, flips, nbr)
    place = place_np(out[0], out[1], len(edges))
    return out, place, *links_of_unitigs_np(edges, flips, nbr, len(edges), out[0], out[1], place)


def link_pairs(link_offsets, targets):
    """[(t, t')] in the arrays' order"""
    lo = [int(x) for x in link_offsets]
    return [(t, int(targets[x])) for t in range(len(lo) - 1) for x in range(lo[t], lo[t + 1])]


def assert_mirror_symmetric(link_offsets, targets):
    """t -> t' is a link iff mirror(t') -> mirror(t) is, with multiplicity"""
    pairs = link_pairs(link_offsets, targets)
    assert sorted(pairs) == sorted((b ^ 1, a ^ 1) for a, b in pairs)
    return pairs
