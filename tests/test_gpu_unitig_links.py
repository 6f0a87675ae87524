"""The unitigs as a graph on the GPU: kmx_count_unitig_links, kmx_count_unitig_select(2) (kmx_count_links.hip) and what the Python
layer builds on them (Unitigs.tips, Context.count_clip_tips(2), Unitigs.write_gfa).

Every comparison is u64 equality of whole arrays with the sequential host reference tests/link_np.py (pinned against brute force
over strings in tests/test_link_np.py).  The reference is fed the host copies of what the device made -- adjacency, unitigs, places,
each compared with its own reference in the tests of its own layer -- so a table of 70 000 entries costs the host one loop over its
oriented unitigs.  The bubble graph is tests/test_gpu_read_paths.py's, the dense, circular and hairpin tables are
tests/test_gpu_count_unitigs.py's.  Every family asserts of its own input that it holds what it is there for."""
import ctypes as C
import io

import numpy as np
import pytest

from tests import link_np, unitig_np
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import random_reads, u64
from tests.test_gpu_count_graph import _dense_reads
from tests.test_gpu_count_unitigs import _circles_reads, _dense8_reads, _hairpin_reads, _table
from tests.test_gpu_read_paths import COMP, Graph, _bubble, _ragged, _rc

pytestmark = pytest.mark.gpu

KS = (5, 6, 15, 31, 33, 34, 63, 64)
POISON = -0x5A5A5A5A5A5A5A5B
E_ARG, E_NOMEM = 1, 6
U64_MAX = 2**64 - 1


class Linked:
    """a table on the device with its adjacency, unitigs and index (all made there) and their host copies"""

    def __init__(self, ctx, k, d_k, d_c, min_count=1, adjacency_min_count=None):
        two = k > 32
        self.ctx, self.k, self.d_k, self.d_c, self.min_count = ctx, k, d_k, d_c, min_count
        self.n = int(d_c.numel())
        adj = ctx.count_adjacency2 if two else ctx.count_adjacency
        self.adj = adj(d_k, d_c, k, min_count, flips=True, neighbors=True)
        self.unitigs = (ctx.count_unitigs2 if two else ctx.count_unitigs)(d_k, d_c, k, min_count, adjacency=self.adj)
        if adjacency_min_count is not None:                                  # (the links are asked of another adjacency than the unitigs')
            self.adj = adj(d_k, d_c, k, adjacency_min_count, flips=True, neighbors=True)
        self.d_place = ctx.count_unitig_index(self.unitigs, self.n)
        self.tk, self.tc = u64(d_k), u64(d_c)
        self.edges, self.flips = self.adj[0].cpu().numpy(), self.adj[1].cpu().numpy()
        self.nbr = u64(self.adj[2])
        self.nodes, self.uoff, self.place = u64(self.unitigs.nodes), u64(self.unitigs.offsets), u64(self.d_place)
        self.U = self.unitigs.n_unitigs
        self._want = None

    def want(self):
        if self._want is None:
            self._want = link_np.links_of_unitigs_np(self.edges, self.flips, self.nbr, self.n, self.nodes, self.uoff, self.place)
        return self._want

    def links(self, **kw):
        return self.ctx.count_unitig_links(self.unitigs, self.adj, self.n, place=self.d_place, **kw)

    def palindromic_unitigs(self):
        pal = unitig_np.palindromes_np(self.tk, self.k)
        first = (self.nodes[self.uoff[:-1].astype(np.int64)] >> np.uint64(1)).astype(np.int64)
        return set(np.nonzero(pal[first])[0].tolist())


_LINKED = {}
_BIG_TABLES = {}


def _linked(ctx, key, make):
    if key not in _LINKED or _LINKED[key].ctx is not ctx:
        _LINKED[key] = make()
    return _LINKED[key]


def _check(x):
    """the device's offsets and targets against the reference's; the mirror symmetry of include/kmx.h on the reference"""
    lo, tg = x.want()
    got = x.links()
    assert got.n_links == len(tg), (x.k, got.n_links, len(tg))
    assert np.array_equal(u64(got.offsets), lo), (x.k, "link offsets")
    assert np.array_equal(u64(got.targets), tg), (x.k, "targets")
    assert np.array_equal(got.degrees.cpu().numpy().reshape(-1), np.diff(lo.astype(np.int64)))
    assert np.array_equal(got.sources().cpu().numpy(), np.array([a for a, _ in link_np.link_pairs(lo, tg)], np.int64))
    pal = x.palindromic_unitigs()
    pairs = link_np.link_pairs(lo, tg)
    if not pal:
        link_np.assert_mirror_symmetric(lo, tg)
    norm = lambda t: t & ~1 if t >> 1 in pal else t
    assert {(norm(a), norm(b)) for a, b in pairs} == {(norm(b ^ 1), norm(a ^ 1)) for a, b in pairs}
    return lo, tg, pairs


def _of_table(ctx, t, min_count=1):
    return _linked(ctx, ("table", id(t), min_count), lambda: Linked(ctx, t.k, t.d_k, t.d_c, min_count))


# ---------------------------------------------------------------- the bubble graph, every k
@pytest.mark.parametrize("k", KS)
def test_links_over_a_bubble(ctx, k):
    gr, g, v = _bubble(ctx, k)
    x = _linked(ctx, ("bubble", k), lambda: Linked(ctx, k, gr.d_k, gr.d_c))
    assert x.U >= 4
    lo, tg, pairs = _check(x)
    deg = np.diff(lo.astype(np.int64))
    assert (deg == 2).any() and (deg == 1).any() and (deg == 0).any()
    if x.U == 4:   # stem, two branches, stem: each stem forks on one side and ends on the other, each branch is linked on both
        assert sorted(deg.tolist()) == [0, 0, 1, 1, 1, 1, 2, 2]
        assert sorted(sorted(d) for d in deg.reshape(-1, 2).tolist()) == [[0, 2], [0, 2], [1, 1], [1, 1]]


# ---------------------------------------------------------------- dense graphs, palindromes, hairpins, self-links
@pytest.mark.parametrize("k", (4, 5, 6, 8))
def test_dense_graph(ctx, k):
    t = _table(ctx, _dense_reads if k < 8 else _dense8_reads, k)
    seen = {"four": False, "pal": False, "hairpin": False, "self": False}
    for min_count in (1, 2):
        x = _of_table(ctx, t, min_count)
        lo, tg, pairs = _check(x)
        pal = x.palindromic_unitigs()
        seen["four"] |= int(np.diff(lo.astype(np.int64)).max()) == 4
        seen["pal"] |= any(b >> 1 in pal for _, b in pairs)
        seen["hairpin"] |= any(a == b ^ 1 for a, b in pairs)
        seen["self"] |= any(a == b for a, b in pairs)
    assert seen["four"] and seen["self"]                                     # sides with four links; t -> t
    assert seen["pal"] == (k % 2 == 0)                                       # links into palindromic one-node unitigs: even k
    assert seen["hairpin"] == (k == 5)                                       # t -> mirror(t): a palindromic overlap of k - 1 bases, odd k


@pytest.mark.parametrize("k", (6, 8))
def test_hairpins(ctx, k):
    """y .. -> palindrome -> .. rc(y): the stem links into the palindrome, both orientations of the palindrome link to the stem's mirror"""
    x = _of_table(ctx, _table(ctx, _hairpin_reads, k))
    lo, tg, pairs = _check(x)
    (p,) = x.palindromic_unitigs()
    assert x.U == 2 and len(pairs) == 3
    (a, b), = [(a, b) for a, b in pairs if a >> 1 != p]
    assert b >> 1 == p and sorted(pairs) == sorted([(a, b), (2 * p, a ^ 1), (2 * p + 1, a ^ 1)])


@pytest.mark.parametrize("k", (15, 31, 33, 47))
def test_circular_sequences(ctx, k):
    x = _of_table(ctx, _table(ctx, _circles_reads, k))
    lo, tg, pairs = _check(x)
    circ = np.nonzero(x.unitigs.circular.cpu().numpy())[0]
    assert len(circ) == 5
    for u in circ.tolist():                                                  # exactly the self-links across the written start
        assert [b for a, b in pairs if a == 2 * u] == [2 * u] and [b for a, b in pairs if a == 2 * u + 1] == [2 * u + 1]


# ---------------------------------------------------------------- past one block and one scan partial
def _big(ctx, k, min_count=1):
    """2400 reads of 100 bases over a sequence of 48 000, 1.2 % of the bases substituted: some 85 000 entries, over 3000 unitigs"""
    def make():
        rng = np.random.default_rng(9100 + k)
        genome = random_reads(rng, 48_000)
        n, L = 2400, 100
        starts = rng.integers(0, len(genome) - L + 1, n)
        starts[:480] = np.arange(480) * 100            # every base is covered
        reads = genome[starts[:, None] + np.arange(L)[None, :]].reshape(-1).copy()
        sub = np.nonzero(rng.random(len(reads)) < 0.012)[0]
        reads[sub] = random_reads(rng, len(sub))
        return (ctx.count_canonical if k <= 31 else ctx.count_canonical2)(ctx.to_device(reads), n, L, k)

    key = ("big table", k)
    if key not in _BIG_TABLES or _BIG_TABLES[key][0] is not ctx:
        _BIG_TABLES[key] = (ctx,) + tuple(make())
    _, d_k, d_c = _BIG_TABLES[key]
    return _linked(ctx, ("big", k, min_count), lambda: Linked(ctx, k, d_k, d_c, min_count))


@pytest.mark.parametrize("k", (31, 47))
def test_more_oriented_unitigs_than_one_partial(ctx, k):
    x = _big(ctx, k)
    assert x.n > 70_000 and 2 * x.U > 4096
    lo, tg, pairs = _check(x)
    deg = np.diff(lo.astype(np.int64))
    first = deg[:4096].sum()
    assert 0 < first < len(tg) and (deg[4096:] > 0).any()                    # links on both sides of the first partial's boundary


# ---------------------------------------------------------------- entries that are not present
@pytest.mark.parametrize("k", (31, 47))
def test_entries_that_are_not_present(ctx, k):
    """unitigs made with min_count = 2; the links asked of that adjacency, and of the adjacency of ALL entries, whose edges into the
    k-mers counted once meet place 0: no link"""
    def table():
        rng = np.random.default_rng(9900 + k)
        g = random_reads(rng, 900)
        v = g.copy()
        v[800] = COMP[v[800]]
        beyond = np.concatenate([g[-(k + 9):], random_reads(rng, 15)])      # seen once: goes on where g ends
        before = np.concatenate([random_reads(rng, 15), g[:k + 9]])
        return Graph(ctx, k, [g, v, beyond, before], times=(2, 2, 1, 1), min_count=2)

    gr = _linked(ctx, ("min2 table", k), table)
    assert (gr.tc == 1).any() and ((gr.place == 0) == (gr.tc < 2)).all()
    x = _linked(ctx, ("min2", k), lambda: Linked(ctx, k, gr.d_k, gr.d_c, 2))
    lo, tg, pairs = _check(x)
    y = _linked(ctx, ("min2 over all edges", k), lambda: Linked(ctx, k, gr.d_k, gr.d_c, 2, adjacency_min_count=1))
    lo2, tg2 = y.want()
    got = y.links()
    assert np.array_equal(u64(got.offsets), lo2) and np.array_equal(u64(got.targets), tg2)
    assert np.array_equal(lo2, lo) and np.array_equal(tg2, tg)              # the edges into absent entries add nothing
    # ... and there are such edges at exit nodes: the input is what the test is about
    met = 0
    for t in range(2 * y.U):
        a, b = int(y.uoff[t >> 1]), int(y.uoff[(t >> 1) + 1])
        v = int(y.nodes[b - 1]) if t & 1 == 0 else int(y.nodes[a]) ^ 1
        for c in range(4):
            e = 4 * (v & 1) + c
            if (int(y.edges[v >> 1]) >> e) & 1 and int(y.place[int(y.nbr.reshape(-1, 8)[v >> 1, e])]) == 0:
                met += 1
    assert met >= 2


# ---------------------------------------------------------------- the call's conventions
def _raw(ctx, x, lo, tg, max_links, n=None, n_unitigs=None, handle="ctx", h=True, **missing):
    """the C call as it is -> (status, *h_n_links)"""
    from kmers_amd.api import _ptr

    a = {"edges": x.adj[0], "flips": x.adj[1], "nbr": x.adj[2], "nodes": x.unitigs.nodes, "offsets": x.unitigs.offsets, "place": x.d_place}
    a.update(missing)
    m = C.c_uint64(12345)
    st = ctx.lib.kmx_count_unitig_links(ctx._h if handle == "ctx" else handle, _ptr(a["edges"]), _ptr(a["flips"]), _ptr(a["nbr"]),
                                        x.n if n is None else n, _ptr(a["nodes"]), _ptr(a["offsets"]), x.U if n_unitigs is None else n_unitigs,
                                        _ptr(a["place"]), _ptr(lo), _ptr(tg), max_links, C.byref(m) if h else None)
    return st, int(m.value)


def test_conventions(ctx):
    import torch

    x = _big(ctx, 31)
    want_lo, want_tg = x.want()
    L = len(want_tg)

    def fresh():
        return (torch.full((2 * x.U + 1,), POISON, dtype=torch.int64, device=ctx.device),
                torch.full((L + 8,), POISON, dtype=torch.int64, device=ctx.device))

    assert _raw(ctx, x, None, None, 0) == (0, L)                             # count only
    lo, tg = fresh()
    assert _raw(ctx, x, lo, tg, L) == (0, L)                                 # exactly enough room; the slots behind stay untouched
    assert np.array_equal(u64(lo), want_lo) and np.array_equal(u64(tg[:L]), want_tg) and (tg[L:] == POISON).all()
    lo2, tg2 = fresh()
    assert _raw(ctx, x, lo2, tg2, L) == (0, L) and torch.equal(lo, lo2) and torch.equal(tg, tg2)   # identical bytes
    lo, tg = fresh()
    assert _raw(ctx, x, lo, tg, L - 1) == (E_NOMEM, L)                       # one short: the offsets all the same
    assert np.array_equal(u64(lo), want_lo) and (tg == POISON).all()
    with pytest.raises(Exception) as e:
        x.links(max_links=L - 1)
    assert getattr(e.value, "status", None) == E_NOMEM
    assert x.links(max_links=L + 5).n_links == L
    made = ctx.count_unitig_links(x.unitigs, x.adj, x.n)                     # the index made on the way
    assert np.array_equal(u64(made.targets), want_tg)
    # a work buffer below the working set: refused before anything runs
    a256 = lambda b: (b + 255) & ~255
    r = (2 * x.U + 1 + 4095) // 4096
    need = a256(4096 * r) + a256(8 * (r + 1))                                # the documented working set (kmx.h)
    lo, tg = fresh()
    try:
        ctx.set_work_buffer_limit(need - 1)
        allocs0 = ctx.work_buffer_info()[1]
        assert _raw(ctx, x, lo, tg, L)[0] == E_NOMEM and ctx.work_buffer_info()[1] == allocs0
        ctx.synchronize()
        assert (lo == POISON).all() and (tg == POISON).all()
        ctx.set_work_buffer_limit(need)                                      # exactly the documented size: served
        assert _raw(ctx, x, lo, tg, L) == (0, L) and np.array_equal(u64(tg[:L]), want_tg)
    finally:
        ctx.set_work_buffer_limit(0)


def test_argument_errors(ctx):
    import torch

    gr, g, v = _bubble(ctx, 31)
    x = _linked(ctx, ("bubble", 31), lambda: Linked(ctx, 31, gr.d_k, gr.d_c))
    L = len(x.want()[1])
    lo = torch.full((2 * x.U + 1,), POISON, dtype=torch.int64, device=ctx.device)
    tg = torch.full((L,), POISON, dtype=torch.int64, device=ctx.device)
    assert _raw(ctx, x, lo, tg, L, handle=None)[0] == E_ARG                  # NULL ctx
    assert _raw(ctx, x, lo, tg, L, h=False)[0] == E_ARG                      # NULL host pointer
    assert _raw(ctx, x, lo, None, L) == (E_ARG, 12345) and _raw(ctx, x, None, tg, L) == (E_ARG, 12345)   # one output NULL
    assert _raw(ctx, x, lo, tg, L, n=2**40 + 1)[0] == E_ARG and _raw(ctx, x, lo, tg, L, n_unitigs=2**40 + 1)[0] == E_ARG
    for name in ("edges", "flips", "nbr", "nodes", "offsets", "place"):
        assert _raw(ctx, x, lo, tg, L, **{name: None})[0] == E_ARG, name
    ctx.synchronize()
    assert (lo == POISON).all() and (tg == POISON).all()                     # nothing ran
    assert _raw(ctx, x, lo, tg, L, n_unitigs=0) == (0, 0)                    # no unitigs: the single offset 0
    assert int(lo[0]) == 0 and (lo[1:] == POISON).all() and (tg == POISON).all()
    lo.fill_(POISON)
    none = dict(edges=None, flips=None, nbr=None, nodes=None, offsets=None, place=None)
    assert _raw(ctx, x, lo, tg, L, n=0, n_unitigs=0, **none) == (0, 0) and (lo == POISON).all()   # nothing at all: a no-op
    assert _raw(ctx, x, None, None, 0, n_unitigs=0) == (0, 0)


@pytest.mark.parametrize("k", (15, 33))
def test_empty_table(ctx, k):
    import torch

    kmers = torch.zeros((0,) if k <= 31 else (0, 2), dtype=torch.int64, device=ctx.device)
    counts = torch.zeros(0, dtype=torch.int64, device=ctx.device)
    x = Linked(ctx, k, kmers, counts)
    got = x.links()
    assert got.n_links == 0 and got.offsets.cpu().tolist() == [0] and got.degrees.shape == (0, 2) and got.sources().numel() == 0
    sk, sc = (ctx.count_unitig_select if k <= 31 else ctx.count_unitig_select2)(kmers, counts, x.unitigs, torch.zeros(0, dtype=torch.uint8, device=ctx.device))
    assert sk.numel() == 0 and sc.numel() == 0
    ck, cc, removed = (ctx.count_clip_tips if k <= 31 else ctx.count_clip_tips2)(kmers, counts, k)
    assert ck.numel() == 0 and cc.numel() == 0 and removed == []


@pytest.mark.parametrize("k", (2, 15, 31, 33, 64))
def test_one_entry(ctx, k):
    """the all-A k-mer is its own successor and its own predecessor: it links to itself on both sides"""
    d_k, d_c = (ctx.count_canonical if k <= 31 else ctx.count_canonical2)(ctx.to_device(np.full(k + 3, ord("A"), np.uint8)), 1, k + 3, k)
    x = Linked(ctx, k, d_k, d_c)
    assert x.n == 1 and x.U == 1
    lo, tg, pairs = _check(x)
    assert lo.tolist() == [0, 1, 2] and tg.tolist() == [0, 1]
    y = Linked(ctx, k, d_k, d_c, 5)                                          # not present: no unitig, the single offset 0
    assert y.U == 0 and y.links().offsets.cpu().tolist() == [0] and y.links().n_links == 0


# ---------------------------------------------------------------- inconsistent inputs
@pytest.mark.parametrize("n", (1000, 70_001))
def test_inconsistent_inputs(ctx, n):
    """random edge, flip and neighbour bytes and random places over valid unitigs: include/kmx.h defines the result, every index is
    checked before it is used, and every target names a unitig"""
    import torch

    from kmers_amd.api import Unitigs

    rng = np.random.default_rng(9300 + n)
    edges, flips = rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 256, n).astype(np.uint8)
    nbr = rng.integers(0, 2**64, (n, 8), dtype=np.uint64)
    near = rng.random((n, 8)) < 0.8
    nbr[near] = rng.integers(0, n + n // 8, int(near.sum())).astype(np.uint64)
    place = rng.integers(0, 8 * (n + n // 8), n).astype(np.uint64)
    place[rng.random(n) < 0.1] = 0
    nodes = (2 * rng.permutation(n) + rng.integers(0, 2, n)).astype(np.uint64)
    nodes[rng.random(n) < 0.01] += np.uint64(2 * n)                         # nodes naming entries beyond the table
    cuts = np.unique(np.concatenate([[0, n], rng.integers(1, n, n // 3)]))
    offsets = cuts.astype(np.uint64)
    n_unitigs = len(offsets) - 1
    want_lo, want_tg = link_np.links_of_unitigs_np(edges, flips, nbr, n, nodes, offsets, place)
    deg = np.diff(want_lo.astype(np.int64))
    assert len(want_tg) > n_unitigs // 8 and deg.max() >= 3 and (want_tg < 2 * n_unitigs).all()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else a).to(ctx.device)
    un = Unitigs(dev(nodes), dev(offsets), None, None, n_unitigs, 31)
    got = ctx.count_unitig_links(un, (dev(edges), dev(flips), dev(nbr)), n, place=dev(place))
    assert np.array_equal(u64(got.offsets), want_lo) and np.array_equal(u64(got.targets), want_tg)
    assert int(got.targets.max()) < 2 * n_unitigs
    # the selection on the same places: a position outside the offsets reads as not kept
    keep = (rng.random(n_unitigs) < 0.5).astype(np.uint8)
    keys, counts = np.arange(n, dtype=np.uint64) * np.uint64(3), rng.integers(1, 9, n).astype(np.uint64)
    sk, sc = link_np.select_np(keys, counts, place, offsets, keep)
    gk, gc = ctx.count_unitig_select(dev(keys), dev(counts), un, dev(keep), place=dev(place))
    assert 0 < len(sk) < n and np.array_equal(u64(gk), sk) and np.array_equal(u64(gc), sc)


# ---------------------------------------------------------------- the selection
@pytest.mark.parametrize("k", (31, 47))
def test_select(ctx, k):
    import torch

    one = k <= 31
    x = _big(ctx, k)
    assert x.n > 2 * 16384                                                   # past one CHUNK of the compaction
    sel = ctx.count_unitig_select if one else ctx.count_unitig_select2
    rng = np.random.default_rng(9400 + k)
    masks = {"random": (rng.random(x.U) < 0.5).astype(np.uint8), "ones": np.ones(x.U, np.uint8), "zeros": np.zeros(x.U, np.uint8)}
    for name, keep in masks.items():
        wk, wc = link_np.select_np(x.tk, x.tc, x.place, x.uoff, keep)
        gk, gc = sel(x.d_k, x.d_c, x.unitigs, ctx.to_device(keep), place=x.d_place)
        assert u64(gk).shape == wk.shape and np.array_equal(u64(gk), wk) and np.array_equal(u64(gc), wc), (k, name)
        if one:                                                              # a table: keys ascending and distinct
            assert (wk[1:] > wk[:-1]).all()
        else:
            assert ((wk[1:, 1] > wk[:-1, 1]) | ((wk[1:, 1] == wk[:-1, 1]) & (wk[1:, 0] > wk[:-1, 0]))).all()
    assert 0 < len(link_np.select_np(x.tk, x.tc, x.place, x.uoff, masks["random"])[1]) < x.n
    gk, gc = sel(x.d_k, x.d_c, x.unitigs, torch.ones(x.U, dtype=torch.bool, device=ctx.device))   # bool mask, index made on the way
    assert np.array_equal(u64(gk), x.tk) and np.array_equal(u64(gc), x.tc)
    # all ones over the unitigs of min_count = m: the filter's [m, 2^64 - 1]
    y = _big(ctx, k, 2)
    assert 0 < int((y.tc >= 2).sum()) < y.n
    gk, gc = sel(y.d_k, y.d_c, y.unitigs, ctx.to_device(np.ones(y.U, np.uint8)), place=y.d_place)
    fk, fc = (ctx.count_filter if one else ctx.count_filter2)(y.d_k, y.d_c, 2, U64_MAX)
    assert torch.equal(gk, fk) and torch.equal(gc, fc)


@pytest.mark.parametrize("k", (31, 47))
def test_select_contract(ctx, k):
    import torch

    from kmers_amd.api import _ptr

    x = _big(ctx, k)
    w = 1 if k <= 31 else 2
    rng = np.random.default_rng(9500 + k)
    keep = (rng.random(x.U) < 0.5).astype(np.uint8)
    wk, wc = link_np.select_np(x.tk, x.tc, x.place, x.uoff, keep)
    m = len(wc)
    d_keep = ctx.to_device(keep)
    km = x.d_k.contiguous().view(-1)
    fn = ctx.lib.kmx_count_unitig_select if w == 1 else ctx.lib.kmx_count_unitig_select2
    ok_ = torch.full((w * (m + 8),), POISON, dtype=torch.int64, device=ctx.device)
    oc = torch.full((m + 8,), POISON, dtype=torch.int64, device=ctx.device)

    def call(keys, out_k, out_c, max_out, n=x.n, place=x.d_place, offsets=x.unitigs.offsets, kp=d_keep, n_unitigs=x.U, handle="ctx"):
        got = C.c_uint64(12345)
        st = fn(ctx._h if handle == "ctx" else handle, _ptr(keys), _ptr(x.d_c), n, _ptr(place), _ptr(offsets), n_unitigs, _ptr(kp), _ptr(out_k),
                _ptr(out_c), max_out, C.byref(got))
        return st, got.value

    assert call(km, ok_, oc, m - 1) == (E_NOMEM, m)                          # one short: the right count, outputs untouched
    assert (ok_ == POISON).all() and (oc == POISON).all()
    assert call(km, None, None, 0) == (0, m)                                 # count only
    assert call(km, ok_, None, m)[0] == E_ARG and call(km, None, oc, m)[0] == E_ARG
    assert call(km, ok_, oc, m, handle=None)[0] == E_ARG
    assert call(km, ok_, oc, m, n=2**38 + 1)[0] == E_ARG and call(km, ok_, oc, m, n_unitigs=2**40 + 1)[0] == E_ARG
    assert call(km, ok_, oc, m, place=None)[0] == E_ARG and call(km, ok_, oc, m, offsets=None)[0] == E_ARG and call(km, ok_, oc, m, kp=None)[0] == E_ARG
    if w == 2:
        assert call(km[1:], ok_, oc, m)[0] == E_ARG and call(km, ok_[1:], oc, m)[0] == E_ARG   # misaligned two-word key arrays
    assert (ok_ == POISON).all() and (oc == POISON).all()
    assert call(km, ok_, oc, m, n_unitigs=0) == (0, 0) and call(km, ok_, oc, m, n=0) == (0, 0)   # nothing to keep
    assert (ok_ == POISON).all() and (oc == POISON).all()
    assert call(km, ok_, oc, m) == (0, m)                                    # exactly the answer; the slots behind it untouched
    assert np.array_equal(u64(ok_[:w * m]).reshape(wk.shape), wk) and np.array_equal(u64(oc[:m]), wc)
    assert (ok_[w * m:] == POISON).all() and (oc[m:] == POISON).all()
    a256 = lambda b: (b + 255) & ~255
    chunks = (x.n + 16383) // 16384
    need = a256(16384 * chunks) + a256(8 * (chunks + 2))                     # the documented working set (kmx.h)
    ok_.fill_(POISON)
    try:
        ctx.set_work_buffer_limit(need - 1)
        assert call(km, ok_, oc, m)[0] == E_NOMEM
        ctx.synchronize()
        assert (ok_ == POISON).all()
        ctx.set_work_buffer_limit(need)
        assert call(km, ok_, oc, m) == (0, m)
    finally:
        ctx.set_work_buffer_limit(0)


# ---------------------------------------------------------------- tip clipping
def clip_input(k):
    """a sequence of 2000 bases, a branch of k // 2 new bases attached in its middle, and a separate sequence of k + 3 bases"""
    rng = np.random.default_rng(9600 + k)
    main = random_reads(rng, 2000)
    mid = 1000
    new = random_reads(rng, k // 2)
    if new[0] == main[mid]:
        new[0] = COMP[new[0]]
    branch = np.concatenate([main[mid - (k - 1):mid], new])
    island = random_reads(rng, k + 3)
    return main, branch, island


@pytest.mark.parametrize("islands", (False, True))
@pytest.mark.parametrize("k", (15, 31, 47))
def test_clip_tips(ctx, k, islands):
    import torch

    one = k <= 31
    main, branch, island = clip_input(k)
    count = ctx.count_canonical if one else ctx.count_canonical2

    def table(seqs):
        bases, offsets = _ragged(seqs)
        return count(ctx.to_device(bases), len(seqs), 0, k, offsets=ctx.to_device(offsets))

    d_k, d_c = table([main, branch, island])
    wk, wc = table([main] if islands else [main, island])
    n_main, n_all = 2000 - k + 1, int(d_c.numel())
    assert n_all == n_main + k // 2 + 4 and int(wc.numel()) == n_main + (0 if islands else 4)   # the input: nothing shared, nothing repeated
    clip = ctx.count_clip_tips if one else ctx.count_clip_tips2
    ck, cc, removed = clip(d_k, d_c, k, islands=islands)
    assert removed == [k // 2 + (4 if islands else 0)]
    assert torch.equal(ck, wk) and torch.equal(cc, wc)
    un = (ctx.count_unitigs if one else ctx.count_unitigs2)(ck, cc, k)
    seqs = [un.sequence(u) for u in range(un.n_unitigs)]
    assert un.n_unitigs == (1 if islands else 2)
    assert bytes(main) in seqs or bytes(_rc(main)) in seqs                   # the fork is gone: the sequence is one unitig again
    ck2, cc2, removed2 = clip(d_k, d_c, k, rounds=3, islands=islands)        # a second round removes nothing, and there is no third
    assert removed2 == [removed[0], 0] and torch.equal(ck2, wk) and torch.equal(cc2, wc)
    same_k, same_c, none = clip(d_k, d_c, k, max_nodes=k // 2 - 1, islands=False)
    assert none == [0] and torch.equal(same_k, d_k) and torch.equal(same_c, d_c)   # a tip longer than max_nodes stays


# ---------------------------------------------------------------- GFA
@pytest.mark.parametrize("k", (31, 47))
def test_write_gfa(ctx, k, tmp_path):
    gr, g, v = _bubble(ctx, k)
    x = _linked(ctx, ("bubble", k), lambda: Linked(ctx, k, gr.d_k, gr.d_c))
    links = x.links()
    out = io.StringIO()
    x.unitigs.write_gfa(out, links)
    lines = out.getvalue().splitlines()
    assert lines[0] == "H\tVN:Z:1.0"
    seg = {}
    for ln in (ln for ln in lines if ln.startswith("S\t")):
        _, name, s, ln_tag, kc = ln.split("\t")
        assert ln_tag == f"LN:i:{len(s)}" and s.encode() == x.unitigs.sequence(int(name)) and kc == f"KC:i:{int(u64(x.unitigs.count_sums)[int(name)])}"
        seg[name] = np.frombuffer(s.encode(), np.uint8)
    assert len(seg) == x.U
    n_lines = 0
    for ln in (ln for ln in lines if ln.startswith("L\t")):
        _, a, sa, b, sb, ov = ln.split("\t")
        assert ov == f"{k - 1}M"
        left = seg[a] if sa == "+" else _rc(seg[a])
        right = seg[b] if sb == "+" else _rc(seg[b])
        assert bytes(left[len(left) - (k - 1):]) == bytes(right[:k - 1])    # the two segments overlap by k - 1 bases as strings
        n_lines += 1
    pairs = link_np.link_pairs(*x.want())
    assert n_lines == (len(pairs) + sum(1 for a, b in pairs if (b ^ 1, a ^ 1) == (a, b))) // 2 and n_lines >= 4
    assert len(lines) == 1 + x.U + n_lines
    x.unitigs.write_gfa(tmp_path / "graph.gfa", links)                       # a path instead of a file object
    assert (tmp_path / "graph.gfa").read_text().splitlines() == lines
