"""Host reference of the count family's graph layer (kmx_count_adjacency(2), kmx_count_edge_histogram, kmx_count_unitig_ends), in
numpy, on top of count_np.host_lookup.  Shared by tests/test_gpu_count_graph.py; pinned against brute force over Python strings in
tests/test_graph_np.py, which needs no GPU.

A table is count_np.table_of's: one-word keys uint64[n], two-word keys uint64[n, 2] rows (low, high), ascending as 2k-bit integers.
All arithmetic here runs on a (low, high) pair of uint64 arrays -- a one-word key is the pair (key, 0) -- straight from the
definitions: the eight neighbouring words are spelled, reverse-complemented, compared and looked up one slot at a time.  Nothing here
knows about groups of consecutive words or which spelling a search can skip.

    S_c(x) = (x >> 2) | (c << (2k - 2))        edge slot c        (Kmer::append_base)
    P_c(x) = ((x << 2) | c) & (4^k - 1)        edge slot 4 + c    (Kmer::prepend_base)
"""
import numpy as np

from tests.count_np import host_lookup

NO_ENTRY = np.uint64(2**64 - 1)
U = np.uint64
_ONE_BIT = np.array([bin(v).count("1") == 1 for v in range(16)])
_LOW_BIT = np.array([(v & -v).bit_length() - 1 if v else 0 for v in range(16)], np.int64)


# ---------------------------------------------------------------- 2k-bit words as (low, high) uint64 arrays
def split(tk):
    """table keys -> (low, high)"""
    tk = np.asarray(tk, np.uint64)
    if tk.ndim == 1:
        return tk.copy(), np.zeros(len(tk), np.uint64)
    return tk[:, 0].copy(), tk[:, 1].copy()


def join(lo, hi, words):
    """(low, high) -> keys in the table's layout"""
    return lo.copy() if words == 1 else np.stack([lo, hi], axis=1)


def mask2(lo, hi, k):
    """the low 2k bits"""
    if 2 * k <= 64:
        return (lo & U((1 << (2 * k)) - 1) if 2 * k < 64 else lo), np.zeros_like(hi)
    return lo, (hi & U((1 << (2 * k - 64)) - 1) if 2 * k < 128 else hi)


def shl_base(lo, hi, k):
    """one base up, the top base dropped"""
    return mask2(lo << U(2), (hi << U(2)) | (lo >> U(62)), k)


def shr_base(lo, hi):
    """one base down, the lowest base dropped"""
    return (lo >> U(2)) | (hi << U(62)), hi >> U(2)


def with_top(lo, hi, k, c):
    """base c at the top position (which holds 0)"""
    s = 2 * k - 2
    if s >= 64:
        return lo, hi | U(c << (s - 64))
    return lo | U(c << s), hi


def _revgroups64(x):
    x = ((x >> U(2)) & U(0x3333333333333333)) | ((x & U(0x3333333333333333)) << U(2))
    x = ((x >> U(4)) & U(0x0F0F0F0F0F0F0F0F)) | ((x & U(0x0F0F0F0F0F0F0F0F)) << U(4))
    return x.byteswap()


def revcomp2(lo, hi, k):
    """reverse complement of a 2k-bit word: the 64 two-bit groups of the complement reversed, then shifted down to 2k bits"""
    rl, rh = _revgroups64(~hi), _revgroups64(~lo)
    s = 128 - 2 * k
    if s >= 64:
        return rh >> U(s - 64), np.zeros_like(rh)
    if s == 0:
        return rl, rh
    return (rl >> U(s)) | (rh << U(64 - s)), rh >> U(s)


def less2(alo, ahi, blo, bhi):
    return (ahi < bhi) | ((ahi == bhi) & (alo < blo))


def neighbour_word(lo, hi, k, e):
    """the word of edge slot e as spelled on the strand of (lo, hi)"""
    c = e & 3
    if e < 4:
        return with_top(*shr_base(lo, hi), k, c)
    l, h = shl_base(lo, hi, k)
    return l | U(c), h


# ---------------------------------------------------------------- the three calls
def adjacency_np(tk, tc, k, min_count=1):
    """-> edges uint8[n], flips uint8[n], nbr uint64[n, 8] (NO_ENTRY where the edge is absent); tc None = every entry present"""
    tk = np.asarray(tk, np.uint64)
    n = len(tk)
    words = 1 if tk.ndim == 1 else 2
    edges, flips = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    nbr = np.full((n, 8), NO_ENTRY, np.uint64)
    if n == 0:
        return edges, flips, nbr
    present = np.ones(n, bool) if tc is None else np.asarray(tc, np.uint64) >= U(min_count)
    lo, hi = split(tk)
    index1 = np.arange(1, n + 1, dtype=np.uint64)   # host_lookup answers index + 1, 0 where the word is no key
    for e in range(8):
        wl, wh = neighbour_word(lo, hi, k, e)
        rl, rh = revcomp2(wl, wh, k)
        flip = less2(rl, rh, wl, wh)
        cl, ch = np.where(flip, rl, wl), np.where(flip, rh, wh)
        hit = host_lookup(tk, index1, join(cl, ch, words))
        j = np.maximum(hit, U(1)) - U(1)
        ok = present & (hit != 0) & present[j.astype(np.int64)]
        edges[ok] |= np.uint8(1 << e)
        flips[ok & flip] |= np.uint8(1 << e)
        nbr[ok, e] = j[ok]
    return edges, flips, nbr


def edge_hist_np(edges):
    return np.bincount(np.asarray(edges, np.uint8), minlength=256).astype(np.uint64)


def unitig_ends_np(edges, flips, nbr):
    """-> uint8[n]: bit 0 = the successor side of the entry ends a non-branching path, bit 1 = the predecessor side does"""
    edges, flips = np.asarray(edges, np.uint8), np.asarray(flips, np.uint8)
    n = len(edges)
    ends = np.zeros(n, np.uint8)
    if n == 0:
        return ends
    nbr = np.asarray(nbr, np.uint64).reshape(n, 8)
    me = np.arange(n)
    for side in (0, 1):
        nib = (edges >> np.uint8(4 * side)) & np.uint8(15)
        one = _ONE_BIT[nib]
        e = 4 * side + _LOW_BIT[nib]
        j = nbr[me, e]
        inside = one & (j < U(n)) & (j != me.astype(np.uint64))
        js = np.where(inside, j, U(0)).astype(np.int64)
        flipped = ((flips >> e.astype(np.uint8)) & np.uint8(1)) != 0
        high = (side == 0) != flipped
        other = np.where(high, edges[js] >> np.uint8(4), edges[js] & np.uint8(15))
        end = ~inside | ~_ONE_BIT[other]
        ends[end] |= np.uint8(1 << side)
    return ends


def graph_summary_np(hist):
    """what kmers_amd.api.GraphSummary derives from the 256 bins, spelled out per edge byte"""
    hist = [int(v) for v in hist]
    out = {"n_edges": 0, "n_isolated": hist[0], "n_tips": 0, "n_branching": 0, "n_interior": 0, "degrees": np.zeros((5, 5), np.int64)}
    for b, v in enumerate(hist):
        o, i = bin(b & 15).count("1"), bin(b >> 4).count("1")
        out["n_edges"] += (o + i) * v
        out["degrees"][i, o] += v
        if b and (o == 0 or i == 0):
            out["n_tips"] += v
        if o > 1 or i > 1:
            out["n_branching"] += v
        if o == 1 and i == 1:
            out["n_interior"] += v
    return out
