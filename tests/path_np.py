"""Host reference of kmx_count_unitig_index and kmx_count_read_paths(2), written straight from the definitions in include/kmx.h: the
place of every entry by one loop over the node list, the segments of every read by one loop over its windows that states the
continuation rule.  Nothing here knows about ballots, scans or slots.  Shared by tests/test_gpu_read_paths.py; pinned against brute
force over Python strings in tests/test_path_np.py, which needs no GPU.

A place is ((p + 1) << 3) | (last << 2) | (first << 1) | o, 0 for an entry in no unitig; a record is (read, length << 32 | start,
unitig, q << 1 | d)."""
import numpy as np

from tests.count_np import host_lookup


def place_np(nodes, offsets, n):
    """-> uint64[n]: where each table entry sits in the unitigs (nodes, offsets)"""
    place = np.zeros(n, np.uint64)
    for u in range(len(offsets) - 1):
        a, b = int(offsets[u]), int(offsets[u + 1])
        for p in range(a, b):
            v = int(nodes[p])
            if (v >> 1) < n:
                place[v >> 1] = ((p + 1) << 3) | ((p == b - 1) << 2) | ((p == a) << 1) | (v & 1)
    return place


def window_places_np(canon, flags, tk, place):
    """-> uint64[windows]: the place of every window's entry, 0 for a window that is invalid, absent or in no unitig"""
    if len(tk) == 0:
        return np.zeros(len(flags), np.uint64)
    return host_lookup(tk, np.asarray(place, np.uint64), canon, flags)


def read_paths_np(canon, flags, win_offsets, tk, place, offsets):
    """-> (path_offsets uint64[n_reads + 1], segments uint64[S, 4]) of the reads whose windows are canon / flags in the slots
    win_offsets (n_reads + 1), against the table keys tk, their places and the unitigs' offsets"""
    n_reads = len(win_offsets) - 1
    n_nodes = int(offsets[-1]) if len(offsets) > 1 else 0
    wp = window_places_np(canon, flags, tk, place) if n_nodes else np.zeros(len(flags), np.uint64)
    segs, path_offsets = [], [0]
    for r in range(n_reads):
        w0, w1 = int(win_offsets[r]), int(win_offsets[r + 1])
        cur = None       # [start, length, unitig, q, d] of the run the previous window is in
        prev = None      # (p, d) of the previous window, None if it is not mapped
        for j in range(w0, w1):
            x = int(wp[j])
            p = (x >> 3) - 1
            if x == 0 or p < 0 or p >= n_nodes:                     # not mapped: it ends a run and starts none
                cur = prev = None
                continue
            o, first, last = x & 1, (x >> 1) & 1, (x >> 2) & 1
            s = 0 if int(flags[j]) & 2 else 1                        # KMX_WIN_FW_CANONICAL: the read spells the key itself
            d = s ^ o
            cont = prev is not None and prev[1] == d and ((d == 0 and p == prev[0] + 1 and not first) or
                                                          (d == 1 and p + 1 == prev[0] and not last))
            if cont:
                cur[1] += 1
            else:
                u = int(np.searchsorted(offsets, np.uint64(p), "right")) - 1
                cur = [j - w0, 1, u, p - int(offsets[u]), d]
                segs.append((r, cur))
            prev = (p, d)
        path_offsets.append(len(segs))
    out = np.zeros((len(segs), 4), np.uint64)
    for i, (r, (start, length, u, q, d)) in enumerate(segs):
        out[i] = (r, (length << 32) | start, u, (q << 1) | d)
    return np.array(path_offsets, np.uint64), out
