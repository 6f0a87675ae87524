"""Host reference of kmx_count_link_support and kmx_count_adjacency_cut, written straight from the definitions in include/kmx.h: one
loop over the pairs of consecutive segments that states the junction and crossing rules, one loop over the oriented unitigs that
walks the exit node's edge bits exactly as tests/link_np.links_of_unitigs_np does and clears the bits of the cut slots.  Nothing here
knows about lanes, atomics or dwords.  Shared by tests/test_gpu_link_support.py; pinned against brute force over Python strings in
tests/test_link_support_np.py, which needs no GPU.

An oriented unitig is t = 2 * u + d; mirror(t) = t ^ 1.  Every array is taken as it comes: any values give the defined result."""
import numpy as np


def _list(link_offsets, targets, t):
    """L(t) as (first slot, [targets]): empty unless the slots lie in the array and are at most four"""
    lo, hi = int(link_offsets[t]), int(link_offsets[t + 1])
    if not (lo <= hi <= len(targets) and hi - lo <= 4):
        return lo, []
    return lo, [int(x) for x in targets[lo:hi]]


def _slot(link_offsets, targets, t, want):
    lo, lst = _list(link_offsets, targets, t)
    return lo + lst.index(want) if want in lst else None


def link_support_np(segments, offsets, link_offsets, targets, support=None, summary=None):
    """-> (support uint64[n_links], summary uint64[3] = junctions, crossed, unlinked), added to the arrays handed in (copies)"""
    segments = np.asarray(segments, np.uint64).reshape(-1, 4)
    n_unitigs = len(offsets) - 1
    support = [0] * len(targets) if support is None else [int(x) for x in support]
    junctions, crossed, unlinked = (0, 0, 0) if summary is None else (int(x) for x in summary)
    size = lambda u: max(int(offsets[u + 1]) - int(offsets[u]), 0)
    rows = [[int(x) for x in row] for row in segments]
    for (r, span, u, pos), (r2, span2, u2, pos2) in zip(rows[:-1], rows[1:]):
        start, length, start2 = span & 0xFFFFFFFF, span >> 32, span2 & 0xFFFFFFFF
        if r2 != r or start2 != start + length:
            continue
        junctions += 1
        q, d, q2, d2 = pos >> 1, pos & 1, pos2 >> 1, pos2 & 1
        slot = None
        if u < n_unitigs and u2 < n_unitigs:
            leaves = q + length == size(u) if d == 0 else q + 1 == length
            enters = q2 == 0 if d2 == 0 else q2 + 1 == size(u2)
            t, t2 = 2 * u + d, 2 * u2 + d2
            if leaves and enters:
                slot = _slot(link_offsets, targets, t, t2)
        if slot is None:
            unlinked += 1
            continue
        crossed += 1
        support[slot] += 1
        mirror = _slot(link_offsets, targets, t2 ^ 1, t ^ 1)
        if mirror is not None and mirror != slot:
            support[mirror] += 1
    return np.array([x % 2**64 for x in support], np.uint64), np.array([junctions, crossed, unlinked], np.uint64)


def adjacency_cut_np(edges, flips, nbr, n, nodes, offsets, place, link_offsets, cut):
    """-> edges_out uint8[n]: the edges with the bit of every cut link slot cleared (the walk of link_np.links_of_unitigs_np)"""
    edges, flips = np.asarray(edges, np.uint8), np.asarray(flips, np.uint8)
    nbr = np.asarray(nbr, np.uint64).reshape(-1, 8)
    out = edges.copy()
    offs = [int(x) for x in offsets]
    n_unitigs = len(offs) - 1
    n_nodes = offs[-1] if n_unitigs else 0
    for t in range(2 * n_unitigs):
        a, b = offs[t >> 1], offs[(t >> 1) + 1]
        if not a < b <= n_nodes:
            continue
        v = int(nodes[b - 1]) if t & 1 == 0 else int(nodes[a]) ^ 1
        i, o = v >> 1, v & 1
        d = 0
        for c in range(4) if i < n else ():
            e = 4 * o + c
            if not (int(edges[i]) >> e) & 1:
                continue
            j = int(nbr[i, e])
            x = int(place[j]) if j < n else 0
            p = (x >> 3) - 1
            if x == 0 or p < 0 or p >= n_nodes:
                continue
            w = o ^ ((int(flips[i]) >> e) & 1)
            if (w == x & 1 and x & 2) or (w != x & 1 and x & 4):
                slot = int(link_offsets[t]) + d
                if slot < len(cut) and cut[slot]:
                    out[i] &= np.uint8(~(1 << e) & 0xFF)
                d += 1
    return out


def unsupported_np(support, min_support=1):
    return (np.asarray(support, np.uint64) < np.uint64(min_support)).astype(np.uint8)
