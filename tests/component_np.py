"""Host reference of kmx_count_unitig_components, written straight from the rule in include/kmx.h: which links are valid, which
unitigs are alive, a union-find over Python integers for the classes, then the roots, ids and records.  Nothing here knows about
lanes, rounds, atomics or the order in which a kernel would look things up.  Shared by tests/test_gpu_unitig_components.py; pinned
against graphs written out by hand, a breadth-first search and scipy in tests/test_component_np.py, which needs no GPU.

With it: the keep formula of UnitigComponents.keep in numpy, Context.count_drop_small_components(2) on the host (the references of
every layer, as clean_np.simplify_np), and the SYNCHRONOUS MODEL of the device's schedule (rounds_model): what the rounds of hook and
jump do when every load of a launch sees the state the launch began with -- the number of rounds DESIGN 4.6.12 quotes."""
import numpy as np

from tests import link_np

NONE = 2**64 - 1
M64 = 2**64 - 1


def valid_lists(link_offsets, targets, U):
    """L(t) for every t < 2 U: the listed targets, or [] unless lo <= hi <= n_links, hi - lo <= 4 and every target is < 2 U"""
    lo = [int(x) for x in np.asarray(link_offsets, np.uint64)]
    tg = [int(x) for x in np.asarray(targets, np.uint64)]
    out = []
    for t in range(2 * U):
        a, b = lo[t], lo[t + 1]
        l = tg[a:b] if a <= b <= len(tg) and b - a <= 4 else []
        out.append(l if all(x < 2 * U for x in l) else [])
    return out


def edges_np(link_offsets, targets, U, mask=None):
    """the adjacency as a set of pairs (u, v), u < v, both alive"""
    alive = [True] * U if mask is None else [int(x) != 0 for x in mask]
    pairs = set()
    for t, l in enumerate(valid_lists(link_offsets, targets, U)):
        u = t >> 1
        for x in l:
            v = x >> 1
            if u != v and alive[u] and alive[v]:
                pairs.add((min(u, v), max(u, v)))
    return pairs, alive


def components_np(offsets, sums, link_offsets, targets, mask=None, U=None):
    """-> (labels u64[U], ids u64[U], records u64[C, 4], C); offsets, sums and mask may be None (then U is given or read off the
    link offsets)"""
    if U is None:
        U = len(offsets) - 1 if offsets is not None else (len(link_offsets) - 1) // 2
    pairs, alive = edges_np(link_offsets, targets, U, mask)
    parent = list(range(U))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, v in pairs:
        a, b = find(u), find(v)
        if a != b:
            parent[max(a, b)] = min(a, b)                                    # (the smaller index stays the root: the root is the minimum)
    offs = None if offsets is None else [int(x) for x in np.asarray(offsets, np.uint64)]

    def m(u):
        if offs is None:
            return 1
        return offs[u + 1] - offs[u] if offs[u + 1] >= offs[u] else 0

    labels = [find(u) if alive[u] else NONE for u in range(U)]
    roots = sorted({l for l in labels if l != NONE})
    rank = {r: i for i, r in enumerate(roots)}
    ids = [rank[l] if l != NONE else NONE for l in labels]
    rec = [[r, 0, 0, 0] for r in roots]
    for u in range(U):
        if alive[u]:
            r = rec[ids[u]]
            r[1] += 1
            r[2] = (r[2] + m(u)) & M64
            r[3] = (r[3] + (m(u) if sums is None else int(np.uint64(sums[u])))) & M64
    return np.array(labels, np.uint64), np.array(ids, np.uint64), np.array(rec, np.uint64).reshape(-1, 4), len(roots)


def keep_np(ids, records, min_nodes=0, min_unitigs=0, min_count_sum=0, largest=None):
    """UnitigComponents.keep on the host: a component stays iff it meets every bound and, with largest=n, is one of the n with the
    most nodes (ties to the smaller id); a unitig with no component is 0"""
    rec = [[int(x) for x in r] for r in np.asarray(records, np.uint64).reshape(-1, 4)]
    ok = [r[2] >= min_nodes and r[1] >= min_unitigs and r[3] >= min_count_sum for r in rec]
    if largest is not None:
        top = set(sorted(range(len(rec)), key=lambda c: (-rec[c][2], c))[:max(largest, 0)])
        ok = [o and c in top for c, o in enumerate(ok)]
    return np.array([1 if int(c) != NONE and ok[int(c)] else 0 for c in np.asarray(ids, np.uint64)], np.uint8)


def drop_small_np(tk, tc, k, min_nodes, min_count=1):
    """Context.count_drop_small_components(2) on the host -> (keys, counts, (labels, ids, records, C))"""
    out, place, lo, tg = link_np.links_of_table_np(tk, tc, k, min_count)
    comp = components_np(out[1], out[3], lo, tg)
    keep = keep_np(comp[1], comp[2], min_nodes=min_nodes)
    return (*link_np.select_np(tk, tc, place, out[1], keep), comp)


def rounds_model(link_offsets, targets, U, mask=None):
    """The device's schedule with every launch reading the state it began with -> (labels as a list, rounds).  A round is a hook --
    for every adjacent pair, parent[max(pu, pv)] = min(itself, min(pu, pv)) -- then one jump, parent[u] = parent[parent[u]]; the
    rounds end with the first that sees no pair of different parents and no parent that is not a root.  (The device's loads may
    see newer values than this; that can only save rounds.)"""
    pairs, alive = edges_np(link_offsets, targets, U, mask)
    e = np.array(sorted(pairs), np.int64).reshape(-1, 2)
    parent = np.arange(U, dtype=np.int64)
    live = np.array(alive, bool)
    rounds = 0
    while True:
        rounds += 1
        pu, pv = parent[e[:, 0]], parent[e[:, 1]]
        differ = pu != pv
        changed = bool(differ.any())
        np.minimum.at(parent, np.maximum(pu, pv)[differ], np.minimum(pu, pv)[differ])
        g = parent[parent]
        changed |= bool((g != parent)[live].any())
        parent = g
        if not changed:
            break
    return [int(p) if a else NONE for p, a in zip(parent, alive)], rounds


def link_arrays(U, directed):
    """Synthetic link arrays (the call reads indices only) -> (link_offsets u64[2 U + 1], targets u64): every pair (u, v) of
    `directed` becomes one link from a side of u that has room (side 0 first) to an orientation of v; at most eight per unitig"""
    lists = [[] for _ in range(2 * U)]
    for u, v in directed:
        side = 2 * u if len(lists[2 * u]) < 4 else 2 * u + 1
        assert len(lists[side]) < 4, (u, "more than eight links")
        lists[side].append(2 * v + ((u + v) & 1))
    lo = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    return lo, np.array([t for l in lists for t in l], np.uint64)


def both_ways(pairs):
    return [p for u, v in pairs for p in ((u, v), (v, u))]
