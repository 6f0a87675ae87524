"""Reads threaded through the unitigs on the GPU: kmx_count_unitig_index and kmx_count_read_paths(2) (kmx_count_paths.hip).

Every comparison is u64 equality of whole arrays -- the places, the path offsets and the (S, 4) records -- with the sequential host
reference tests/path_np.py (pinned against brute force over strings in tests/test_path_np.py), fed the oracle's canonical words and
flags of the batch.  The graph is a random sequence and a copy with one substitution (a bubble: at least four unitigs), counted and
compacted on the device; the substitution sits near the end so that long reads fit in front of it.  At k = 5 and 6 the sequence is
drawn without a repeated (k - 1)-mer, or nothing longer than a few nodes would be a unitig.  Reads are pieces of the two sequences,
forward and reverse-complemented, some with a substituted base or an N, and a share of random reads that lie nowhere.
Every check asserts of its own input what the docstring of _assert_input lists, and that the segment lengths add up to the non-zero
answers of count_lookup_reads(2) with the places as the counts.  A table and its unitigs are made once per module and shared."""
import ctypes as C

import numpy as np
import pytest

from tests import path_np
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import orc_windows, random_reads, u64

pytestmark = pytest.mark.gpu

KS = (5, 6, 15, 31, 33, 34, 63, 64)
POISON = -0x5A5A5A5A5A5A5A5B
E_ARG, E_K_RANGE, E_NOMEM = 1, 2, 6
COMP = np.zeros(256, np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")


def _rc(s):
    return COMP[s[::-1]]


def _canon_code(s):
    a, b = bytes(s), bytes(_rc(s))
    return min(a[::-1], b[::-1])


def _genome(rng, k, length):
    """a random sequence; at k < 15 no (k - 1)-mer occurs twice on either strand and none is its own reverse complement -- either
    would be a branch (greedy, drawn again when it gets stuck)"""
    if k >= 15:
        return random_reads(rng, length)
    letters = np.frombuffer(b"ACGT", np.uint8)
    while True:
        s, seen = list(rng.choice(letters, k - 2)), set()
        while len(s) < length:
            for c in rng.permutation(letters):
                w = np.array(s[len(s) - (k - 2):] + [c], np.uint8)
                key = _canon_code(w)
                if key not in seen and bytes(w) != bytes(_rc(w)):
                    seen.add(key)
                    s.append(c)
                    break
            else:
                break
        if len(s) == length:
            return np.array(s, np.uint8)


def _ragged(seqs):
    offsets = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
    return (np.concatenate(seqs) if sum(len(s) for s in seqs) else np.zeros(0, np.uint8)).astype(np.uint8), offsets


class Graph:
    """sequences counted on the device (each `times` over), the unitigs of the table and their index, with host copies"""

    def __init__(self, ctx, k, seqs, times=1, min_count=1):
        self.ctx, self.k, self.seqs = ctx, k, seqs
        bases, offsets = _ragged([s for s, t in zip(seqs, times if isinstance(times, tuple) else (times,) * len(seqs)) for _ in range(t)])
        two = k > 32
        self.d_k, self.d_c = (ctx.count_canonical2 if two else ctx.count_canonical)(ctx.to_device(bases), len(offsets) - 1, 0, k, offsets=ctx.to_device(offsets))
        self.n = int(self.d_c.numel())
        self.unitigs = (ctx.count_unitigs2 if two else ctx.count_unitigs)(self.d_k, self.d_c, k, min_count)
        self.d_place = ctx.count_unitig_index(self.unitigs, self.n)
        self.tk, self.tc = u64(self.d_k), u64(self.d_c)
        self.nodes, self.uoff = u64(self.unitigs.nodes), u64(self.unitigs.offsets)
        self.place = path_np.place_np(self.nodes, self.uoff, self.n)


_GRAPHS = {}


def _bubble(ctx, k, length=None):
    """the bubble graph of k: (graph, sequence, variant)"""
    length = length or (70 if k == 5 else 250 if k == 6 else 900)
    key = ("bubble", k, length)
    if key not in _GRAPHS or _GRAPHS[key][0].ctx is not ctx:
        rng = np.random.default_rng(9100 + k)
        at = length - length // 9
        while True:
            g = _genome(rng, k, length)
            v = g.copy()
            v[at] = COMP[v[at]]
            if k >= 15:
                break
            # (small k: the substitution's own (k - 1)-mers must be new as well, or the bubble is not the only branch)
            old = {_canon_code(g[i:i + k - 1]) for i in range(length - k + 2)}
            new = [v[i:i + k - 1] for i in range(at - k + 2, at + 1)]
            if len({_canon_code(w) for w in new} | old) == len(old) + len(new) and all(bytes(w) != bytes(_rc(w)) for w in new):
                break
        _GRAPHS[key] = (Graph(ctx, k, [g, v]), g, v)
    return _GRAPHS[key]


def _make_reads(rng, g, v, k, lens):
    """pieces of the sequence and its variant, by length: every second one reverse-complemented, every fourth random (it lies nowhere),
    some with a substituted base in the middle or an N; then a clean piece from the start and one across the bubble"""
    out = []
    for i, L in enumerate(int(x) for x in lens):
        L = min(L, len(g))
        src = v if i % 3 == 1 else g
        a = int(rng.integers(0, len(g) - L + 1))
        r = src[a:a + L].copy()
        if i % 4 == 3:
            r = random_reads(rng, L)
        elif L:
            if i % 5 == 0:
                r[L // 2] = COMP[r[L // 2]]
            if i % 11 == 0:
                r[L // 3] = ord("N")
            if i % 2:
                r = _rc(r)
        out.append(r)
    if len(out) >= 2:
        L0, L1 = len(out[0]), len(out[1])
        out[0] = g[:L0].copy()
        end = min(len(g), len(g) - len(g) // 9 + L1 // 2)
        out[1] = g[end - L1:end].copy()
    return out


def _call_raw(ctx, k, bases, n_reads, L, d_off, d_k, n, d_place, d_uoff, n_unitigs, d_po, d_segs, max_segments):
    """the C call as it is -> (status, *h_n_segments)"""
    from kmers_amd import api

    fn = ctx.lib.kmx_count_read_paths if k <= 31 else ctx.lib.kmx_count_read_paths2
    r = ctx._reads(bases, n_reads, L, d_off)
    s = C.c_uint64(12345)
    st = fn(ctx._h, C.byref(r), k, api._ptr(d_k), n, api._ptr(d_place), api._ptr(d_uoff), n_unitigs, api._ptr(d_po), api._ptr(d_segs), max_segments,
            C.byref(s))
    return st, int(s.value)


def _assert_input(recs, po, wp, flags, wo):
    """what every test asks of its own input: a read with one segment over all its windows, a read with at least three segments, a
    segment with d = 1, a segment with q > 0, a tenth of the valid windows mapped and a tenth unmapped"""
    nwin = np.diff(wo.astype(np.int64))
    nseg = np.diff(po.astype(np.int64))
    length = (recs[:, 1] >> np.uint64(32)).astype(np.int64)
    first = po[:-1].astype(np.int64)
    one = (nseg == 1) & (nwin > 0)
    assert (length[first[one]] == nwin[one]).any(), "no read with one segment over all its windows"
    assert (nseg >= 3).any(), "no read with three segments"
    assert (recs[:, 3] & np.uint64(1)).any(), "no segment with d = 1"
    assert ((recs[:, 3] >> np.uint64(1)) > 0).any(), "no segment with q > 0"
    valid = (flags & 1) != 0
    nv, mapped = int(valid.sum()), int((wp[valid] != 0).sum())
    assert nv > 0 and 10 * mapped >= nv and 10 * (nv - mapped) >= nv, (nv, mapped)


def _check(ctx, orc, gr, host, n, L, offsets=None, shift=0, conditions=True):
    """device places, path offsets and records against the host reference; returns (path offsets, records, window offsets)"""
    k = gr.k
    assert np.array_equal(u64(gr.d_place), gr.place)
    canon, flags = orc_windows(orc, host, n, L, k, offsets)
    wo = orc.win_offsets_for(n, L, k, None if offsets is None else np.asarray(offsets, np.uint64))
    want_po, want = path_np.read_paths_np(canon, flags, wo, gr.tk, gr.place, gr.uoff)
    buf = ctx.to_device(np.concatenate([np.zeros(shift, np.uint8), host, np.zeros(16, np.uint8)]))
    bases = buf[shift:shift + len(host)]
    d_off = None if offsets is None else ctx.to_device(np.asarray(offsets, np.uint64))
    f = ctx.count_read_paths if k <= 31 else ctx.count_read_paths2
    got = f(bases, n, L, k, gr.d_k, gr.unitigs, place=gr.d_place, offsets=d_off)
    assert got.n_segments == len(want), (k, n, L, got.n_segments, len(want))
    assert np.array_equal(u64(got.offsets), want_po), (k, n, L, "path offsets")
    g = u64(got.segments)
    bad = np.nonzero((g != want).any(axis=1))[0]
    assert len(bad) == 0, (k, n, L, shift, bad[:5], g[bad[:2]], want[bad[:2]])
    # the views, and the windows per unitig
    assert np.array_equal(got.read.cpu().numpy().view(np.uint64), want[:, 0])
    assert np.array_equal((got.start + (got.length << 32)).cpu().numpy().view(np.uint64), want[:, 1])
    assert np.array_equal(((got.pos << 1) | got.reverse.long()).cpu().numpy().view(np.uint64), want[:, 3])
    cov = np.zeros(gr.unitigs.n_unitigs, np.int64)
    np.add.at(cov, want[:, 2].astype(np.int64), (want[:, 1] >> np.uint64(32)).astype(np.int64))
    assert np.array_equal(got.unitig_coverage(gr.unitigs.n_unitigs).cpu().numpy(), cov)
    if conditions:
        # the invariant: the segments' windows are the non-zero answers of the lookup with the places as the counts
        lk = ctx.count_lookup_reads if k <= 31 else ctx.count_lookup_reads2
        answers = u64(lk(bases, n, L, k, gr.d_k, gr.d_place, offsets=d_off))
        assert int((answers != 0).sum()) == int((want[:, 1] >> np.uint64(32)).sum())
        _assert_input(want, want_po, path_np.window_places_np(canon, flags, gr.tk, gr.place), flags, wo)
    return want_po, want, wo


# ---------------------------------------------------------------- the graph and the reads, every k
@pytest.mark.parametrize("k", KS)
def test_ragged_reads_over_a_bubble(ctx, orc, k):
    """reads of 40 .. 150 bases, a read shorter than k, an empty one, one of k bases; a bound of 150, no bound, an odd d_bases"""
    gr, g, v = _bubble(ctx, k)
    assert gr.unitigs.n_unitigs >= 4
    rng = np.random.default_rng(9200 + k)
    lens = np.concatenate([[100, 150], rng.integers(40, 151, 200), [k - 1, 0, k, k + 1, 150]])
    host, offsets = _ragged(_make_reads(rng, g, v, k, lens))
    n = len(lens)
    _check(ctx, orc, gr, host, n, 150, offsets)
    _check(ctx, orc, gr, host, n, 0, offsets, conditions=False)
    _check(ctx, orc, gr, host, n, 150, offsets, shift=1, conditions=False)


@pytest.mark.parametrize("k", KS)
def test_uniform_reads_over_a_bubble(ctx, orc, k):
    gr, g, v = _bubble(ctx, k)
    rng = np.random.default_rng(9300 + k)
    n, L = 150, 40 if k < 15 else 150
    host, _ = _ragged(_make_reads(rng, g, v, k, [L] * n))
    _check(ctx, orc, gr, host, n, L)
    _check(ctx, orc, gr, host, n, L, shift=1, conditions=False)


# ---------------------------------------------------------------- the routes of long reads
@pytest.mark.parametrize("k", (15, 31, 47))
def test_uniform_700_segment_route(ctx, orc, k):
    gr, g, v = _bubble(ctx, k)
    rng = np.random.default_rng(9400 + k)
    n, L = 8, 700
    host, _ = _ragged(_make_reads(rng, g, v, k, [L] * n))
    _check(ctx, orc, gr, host, n, L)
    _check(ctx, orc, gr, host, n, L, shift=1, conditions=False)


@pytest.mark.parametrize("k", (15, 31, 47))
def test_ragged_long_reads_with_a_bound_above_256(ctx, orc, k):
    gr, g, v = _bubble(ctx, k)
    rng = np.random.default_rng(9500 + k)
    lens = np.concatenate([[700, 800], rng.integers(40, 151, 60), [900, 0, 257, 300, k + 255, k + 256, 600, k - 1]])
    host, offsets = _ragged(_make_reads(rng, g, v, k, lens))
    _check(ctx, orc, gr, host, len(lens), 5000, offsets)
    _check(ctx, orc, gr, host, len(lens), 0, offsets, conditions=False)


# ---------------------------------------------------------------- past one chunk
@pytest.mark.parametrize("k", (31, 47))
def test_past_one_chunk(ctx, orc, k):
    """more than 3 * 16384 windows, and reads of 5000 bases whose one run crosses the 4096- and 16384-window boundaries of the scan"""
    gr, g, v = _bubble(ctx, k, 6000)
    rng = np.random.default_rng(9600 + k)
    n, L = 3 * 16384 // (150 - k + 1) + 8, 150
    host, _ = _ragged(_make_reads(rng, g, v, k, [L] * n))
    assert n * (L - k + 1) > 3 * 16384
    _check(ctx, orc, gr, host, n, L)
    lens = np.array([150] * 130 + [5000, 150, 5000, 5000] + [150] * 40)
    reads = _make_reads(rng, g, v, k, lens)
    reads[130] = g[:5000].copy()
    reads[132] = _rc(g[200:5200])
    host, offsets = _ragged(reads)
    po, recs, wo = _check(ctx, orc, gr, host, len(lens), 5000, offsets)
    j0 = wo[recs[:, 0].astype(np.int64)].astype(np.int64) + (recs[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    j1 = j0 + (recs[:, 1] >> np.uint64(32)).astype(np.int64) - 1
    assert (j0 // 4096 != j1 // 4096).any() and (j0 // 16384 != j1 // 16384).any()
    assert ((j1 - j0 + 1) == 5000 - k + 1).any()


# ---------------------------------------------------------------- a cycle
@pytest.mark.parametrize("k", (5, 31, 47))
def test_reads_round_a_cycle(ctx, orc, k):
    """a circular sequence and reads of 2.5 laps: a new segment at every passage of the written start"""
    key = ("circle", k)
    m = 60 if k == 5 else 300
    if key not in _GRAPHS or _GRAPHS[key][0].ctx is not ctx:
        rng = np.random.default_rng(9700 + k)
        circle = _genome(rng, k, m)
        if k == 5:   # (close the circle without a repeated 4-mer: draw until the seam adds none)
            while len({_canon_code(np.concatenate([circle, circle])[i:i + k - 1]) for i in range(m)}) < m:
                circle = _genome(rng, k, m)
        _GRAPHS[key] = (Graph(ctx, k, [np.concatenate([circle, circle[:k - 1]])]), circle)
    gr, circle = _GRAPHS[key]
    assert gr.unitigs.n_unitigs == 1 and int(gr.unitigs.circular[0]) == 1 and gr.unitigs.n_nodes == m
    rng = np.random.default_rng(9800 + k)
    four = np.concatenate([circle] * 4)
    laps = [four[a:a + 2 * m + m // 2 + k - 1] for a in (3, m // 4, m // 2)]
    reads = laps + [_rc(x) for x in laps] + [four[a:a + m // 3 + k] for a in range(0, m, m // 5)] + [random_reads(rng, 2 * m) for _ in range(3)]
    host, offsets = _ragged(reads)
    po, recs, wo = _check(ctx, orc, gr, host, len(reads), 0, offsets)
    for r in range(6):
        mine = recs[int(po[r]):int(po[r + 1])]
        length = (mine[:, 1] >> np.uint64(32)).astype(np.int64)
        assert len(mine) in (3, 4) and int(length.sum()) == 2 * m + m // 2 and (length == m).any()
        d = mine[:, 3] & np.uint64(1)
        assert ((mine[1:, 3] >> np.uint64(1)) == np.where(d[1:] == 0, 0, m - 1).astype(np.uint64)).all()


# ---------------------------------------------------------------- entries that are not present
@pytest.mark.parametrize("k", (31, 47))
def test_singletons_are_in_no_unitig(ctx, orc, k):
    """unitigs made with min_count = 2: the windows of k-mers counted once are unmapped"""
    key = ("min2", k)
    if key not in _GRAPHS or _GRAPHS[key][0].ctx is not ctx:
        rng = np.random.default_rng(9900 + k)
        g = random_reads(rng, 900)
        v = g.copy()
        v[800] = COMP[v[800]]
        once = random_reads(rng, 400)
        _GRAPHS[key] = (Graph(ctx, k, [g, v, once], times=(2, 2, 1), min_count=2), g, v, once)
    gr, g, v, once = _GRAPHS[key]
    assert (gr.tc == 1).any() and ((gr.place == 0) == (gr.tc < 2)).all()
    rng = np.random.default_rng(9950 + k)
    reads = _make_reads(rng, g, v, k, np.concatenate([[100, 150], rng.integers(40, 151, 120)]))
    reads = [r if i % 4 != 3 else once[(a := int(rng.integers(0, 250))):a + len(r)] for i, r in enumerate(reads)]   # the random reads: pieces seen once
    reads += [np.concatenate([g[:100], once[:100]]), once]
    host, offsets = _ragged(reads)
    po, recs, wo = _check(ctx, orc, gr, host, len(reads), 0, offsets)
    assert int(po[-1]) == int(po[-2])                                                   # `once` itself: no segment
    last = recs[int(po[-3]):int(po[-2])]
    assert len(last) == 1 and int(last[0, 1]) == ((100 - k + 1) << 32)                  # the half that is present, and only it


# ---------------------------------------------------------------- the index on its own
def test_unitig_index_conventions(ctx):
    import torch

    gr, g, v = _bubble(ctx, 31)
    lib, h = ctx.lib, ctx._h
    from kmers_amd.api import _ptr

    fewer = gr.n - 7                                                                     # nodes naming an entry >= n are skipped
    out = torch.full((gr.n,), POISON, dtype=torch.int64, device=ctx.device)
    assert lib.kmx_count_unitig_index(h, _ptr(gr.unitigs.nodes), _ptr(gr.unitigs.offsets), gr.unitigs.n_unitigs, fewer, _ptr(out)) == 0
    assert np.array_equal(u64(out[:fewer]), path_np.place_np(gr.nodes, gr.uoff, fewer)) and (out[fewer:] == POISON).all()
    out.fill_(POISON)
    assert lib.kmx_count_unitig_index(h, None, None, 0, gr.n, _ptr(out)) == 0 and (out == 0).all()   # no unitigs: n zeros
    assert lib.kmx_count_unitig_index(h, None, None, 0, 0, None) == 0
    assert lib.kmx_count_unitig_index(h, _ptr(gr.unitigs.nodes), _ptr(gr.unitigs.offsets), gr.unitigs.n_unitigs, gr.n, None) == E_ARG
    assert lib.kmx_count_unitig_index(h, None, _ptr(gr.unitigs.offsets), gr.unitigs.n_unitigs, gr.n, _ptr(out)) == E_ARG
    one = ctx.count_unitig_index(gr.unitigs, gr.n)
    assert torch.equal(one, gr.d_place) and (one != 0).all()


# ---------------------------------------------------------------- the call's conventions
@pytest.mark.parametrize("k", (31, 47))
def test_conventions(ctx, orc, k):
    import torch

    gr, g, v = _bubble(ctx, k)
    rng = np.random.default_rng(9990 + k)
    n, L = 60, 100
    host, _ = _ragged(_make_reads(rng, g, v, k, [L] * n))
    want_po, want, _ = _check(ctx, orc, gr, host, n, L, conditions=False)
    S = len(want)
    bases = ctx.to_device(host)
    U, d_uoff = gr.unitigs.n_unitigs, gr.unitigs.offsets
    f = ctx.count_read_paths if k <= 31 else ctx.count_read_paths2

    def fresh():
        return (torch.full((n + 1,), POISON, dtype=torch.int64, device=ctx.device),
                torch.full((4 * S,), POISON, dtype=torch.int64, device=ctx.device))

    def raw(po, segs, max_segments, kk=k, n_reads=n, n_tab=gr.n, n_unitigs=U):
        return _call_raw(ctx, kk, bases, n_reads, L, None, gr.d_k, n_tab, gr.d_place, d_uoff, n_unitigs, po, segs, max_segments)

    assert raw(None, None, 0) == (0, S)                                                  # count only
    po, segs = fresh()
    assert raw(po, segs, S) == (0, S)                                                    # exactly enough room
    assert np.array_equal(u64(po), want_po) and np.array_equal(u64(segs).reshape(-1, 4), want)
    po2, segs2 = fresh()
    assert raw(po2, segs2, S) == (0, S) and torch.equal(po, po2) and torch.equal(segs, segs2)   # identical bytes
    po, segs = fresh()
    assert raw(po, segs, S - 1) == (E_NOMEM, S)                                          # one short: the offsets all the same
    assert np.array_equal(u64(po), want_po) and (segs == POISON).all()
    with pytest.raises(Exception) as e:
        f(bases, n, L, k, gr.d_k, gr.unitigs, place=gr.d_place, max_segments=S - 1)
    assert getattr(e.value, "status", None) == E_NOMEM
    assert f(bases, n, L, k, gr.d_k, gr.unitigs, max_segments=S + 5).n_segments == S    # the index made on the way
    po, segs = fresh()
    assert raw(po, None, S) == (E_ARG, 12345) and raw(None, segs, S) == (E_ARG, 12345)   # one output NULL
    assert (po == POISON).all() and (segs == POISON).all()
    for bad_k in (1, 32):
        from kmers_amd.api import _ptr

        r = ctx._reads(bases, n, L, None)
        s = C.c_uint64(0)
        for fn in (ctx.lib.kmx_count_read_paths, ctx.lib.kmx_count_read_paths2):
            assert fn(ctx._h, C.byref(r), bad_k, _ptr(gr.d_k), gr.n, _ptr(gr.d_place), _ptr(d_uoff), U, _ptr(po), _ptr(segs), S, C.byref(s)) == E_K_RANGE
    assert raw(po, segs, S, n_reads=0) == (0, 0) and (po == POISON).all()               # n_reads == 0: a no-op
    assert raw(po, segs, S, n_tab=0) == (0, 0) and (po == 0).all() and (segs == POISON).all()   # an empty table: no segment, every offset 0
    po.fill_(POISON)
    assert raw(po, segs, S, n_unitigs=0) == (0, 0) and (po == 0).all() and (segs == POISON).all()
    # a work buffer below the working set: refused before anything runs
    def a256(b):
        return (b + 255) & ~255

    n_win = n * (L - k + 1)                                                              # the documented working set (kmx.h)
    groups = (n_win + 63) // 64
    need = (a256(8 * n_win) + a256(n_win) + 2 * a256(8 * groups) + a256(4 * groups) + a256(8 * ((n_win + 4095) // 4096 + 2))
            + (a256(16 * n_win) if k > 31 else 0))
    po, segs = fresh()
    try:
        ctx.set_work_buffer_limit(need - 1)
        allocs0 = ctx.work_buffer_info()[1]
        assert raw(po, segs, S)[0] == E_NOMEM and ctx.work_buffer_info()[1] == allocs0   # refused before the buffer was touched
        ctx.synchronize()
        assert (po == POISON).all() and (segs == POISON).all()
        ctx.set_work_buffer_limit(need)                                                  # exactly the documented size: served
        assert raw(po, segs, S) == (0, S) and np.array_equal(u64(segs).reshape(-1, 4), want)
    finally:
        ctx.set_work_buffer_limit(0)
    assert raw(po, segs, S) == (0, S) and np.array_equal(u64(segs).reshape(-1, 4), want)
