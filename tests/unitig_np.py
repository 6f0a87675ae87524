"""Host reference of kmx_count_unitigs(2) and kmx_count_unitig_sequences(2), written straight from the definitions in include/kmx.h
on top of tests/graph_np.py: the links one oriented node at a time, then every chain and every cycle walked node by node.  Nothing
here knows about pointer jumping, scans or scatters.  Shared by tests/test_gpu_count_unitigs.py; pinned against brute force over
Python strings in tests/test_unitig_np.py, which needs no GPU.

An oriented node is v = 2 * entry + o (o = 1: the entry read as its reverse complement); mirror(v) = v ^ 1."""
import numpy as np

from tests import graph_np

_LOW_BIT = [(v & -v).bit_length() - 1 if v else 0 for v in range(16)]
LETTERS = b"ACGT"


def palindromes_np(tk, k):
    """bool[n]: the key is its own reverse complement (even k only)"""
    lo, hi = graph_np.split(tk)
    if k % 2:
        return np.zeros(len(lo), bool)
    rl, rh = graph_np.revcomp2(lo, hi, k)
    return (rl == lo) & (rh == hi)


def links_np(tk, tc, k, min_count, edges, flips, nbr):
    """-> nxt int64[2n]: next(v), -1 where there is none.  tk may be None at odd k; tc None = every entry present."""
    edges, flips = np.asarray(edges, np.uint8), np.asarray(flips, np.uint8)
    n = len(edges)
    nbr = np.asarray(nbr, np.uint64).reshape(n, 8)
    present = np.ones(n, bool) if tc is None else np.asarray(tc, np.uint64) >= np.uint64(min_count)
    ends = graph_np.unitig_ends_np(edges, flips, nbr)
    pal = palindromes_np(tk, k) if k % 2 == 0 else np.zeros(n, bool)
    cand = [-1] * (2 * n)
    for v in range(2 * n):
        i, o = v >> 1, v & 1
        if not present[i] or (int(ends[i]) >> o) & 1:
            continue
        e = 4 * o + _LOW_BIT[(int(edges[i]) >> (4 * o)) & 15]
        j = int(nbr[i, e])
        if j >= n or pal[i] or pal[j]:
            continue
        cand[v] = 2 * j + (o ^ ((int(flips[i]) >> e) & 1))
    nxt = np.full(2 * n, -1, np.int64)
    for v in range(2 * n):
        w = cand[v]
        if w >= 0 and cand[w ^ 1] == v ^ 1:   # the link is mutual
            nxt[v] = w
    return nxt, present


def unitigs_np(tk, tc, k, min_count, edges, flips, nbr):
    """-> nodes uint64[n_nodes], offsets uint64[U + 1], circular uint8[U], count_sums uint64[U]"""
    nxt, present = links_np(tk, tc, k, min_count, edges, flips, nbr)
    n2 = len(nxt)
    prev = [int(nxt[v ^ 1]) ^ 1 if nxt[v ^ 1] >= 0 else -1 for v in range(n2)]
    seen = np.zeros(n2, bool)
    found = []   # (head entry, nodes, circular)
    for v in range(n2):   # chains: from every head along next
        if not present[v >> 1] or prev[v] >= 0:
            continue
        chain = [v]
        while nxt[chain[-1]] >= 0:
            chain.append(int(nxt[chain[-1]]))
            assert len(chain) <= n2
        seen[chain] = True
        head, tail = chain[0], chain[-1]
        if head >> 1 < tail >> 1 or (head >> 1 == tail >> 1 and head & 1 == 0):
            found.append((head >> 1, chain, 0))
    for v in range(n2):   # what is left lies on cycles; ascending, so v is the smallest node of a cycle not seen yet
        if not present[v >> 1] or seen[v]:
            continue
        cycle = [v]
        while int(nxt[cycle[-1]]) != v:
            cycle.append(int(nxt[cycle[-1]]))
            assert nxt[cycle[-1]] >= 0 and len(cycle) <= n2
        seen[cycle] = True
        if v & 1 == 0:   # the cycle that holds 2 i*, i* its smallest entry; the other one of the pair starts at 2 i* + 1
            found.append((v >> 1, cycle, 1))
    found.sort(key=lambda u: u[0])
    counts = None if tc is None else [int(c) for c in np.asarray(tc, np.uint64)]
    nodes = np.array([v for _, c, _ in found for v in c], np.uint64)
    offsets = np.cumsum([0] + [len(c) for _, c, _ in found]).astype(np.uint64)
    circular = np.array([c for _, _, c in found], np.uint8)
    sums = np.array([(len(c) if counts is None else sum(counts[v >> 1] for v in c)) % 2**64 for _, c, _ in found], np.uint64)
    return nodes, offsets, circular, sums


def oriented_words(tk, k):
    """-> [forward words, reverse-complement words] as Python ints per entry"""
    lo, hi = graph_np.split(tk)
    rl, rh = graph_np.revcomp2(lo, hi, k)
    return ([int(a) | (int(b) << 64) for a, b in zip(lo, hi)], [int(a) | (int(b) << 64) for a, b in zip(rl, rh)])


def sequences_np(tk, k, nodes, offsets):
    """-> uint8[n_nodes + U (k - 1)], ASCII: unitig u at byte offsets[u] + u (k - 1)"""
    words = oriented_words(tk, k)
    out = bytearray()
    for u in range(len(offsets) - 1):
        for t in range(int(offsets[u]), int(offsets[u + 1])):
            v = int(nodes[t])
            w = words[v & 1][v >> 1]
            if t == int(offsets[u]):
                out += bytes(LETTERS[(w >> (2 * b)) & 3] for b in range(k))
            else:
                out.append(LETTERS[(w >> (2 * k - 2)) & 3])
    return np.frombuffer(bytes(out), np.uint8)
