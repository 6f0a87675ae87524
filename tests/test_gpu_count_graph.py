"""A count table as the node set of a de Bruijn graph on the GPU: kmx_count_adjacency(2), kmx_count_edge_histogram and
kmx_count_unitig_ends (kmx_count_graph.hip).

Everything is exact: every byte and word of every output is compared with the host reference tests/graph_np.py (numpy, straight
from the definitions, pinned against brute force over strings in tests/test_graph_np.py).  The tables are what
Context.count_canonical(2) makes of seeded reads; a table's device arrays, host copies and reference are made once per module and
shared.  Every case also runs the edge histogram against np.bincount and the unitig ends against the reference, with and without
the directory (a work-buffer cap that leaves no room for it): both routes must give identical bytes."""
import ctypes as C

import numpy as np
import pytest

from tests import graph_np
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import random_reads, u64

pytestmark = pytest.mark.gpu

DENSE_KS = (4, 5, 6)
SPARSE_KS = (15, 21, 31, 33, 47, 63, 64)
NO_ENTRY = 2**64 - 1


# ---------------------------------------------------------------- the read batches
def _dense_reads(k):
    """64 reads of 40 bases: at k <= 6 nearly every canonical k-mer occurs"""
    return random_reads(np.random.default_rng(4100 + k), 64 * 40), 64, 40


def _sparse_reads(k):
    """300 reads of 100 bases cut with overlap from one sequence of 3000: long non-branching paths; 2 % of the bases substituted:
    tips and bubbles; a few N"""
    rng = np.random.default_rng(4200 + k)
    genome = random_reads(rng, 3000)
    n, L = 300, 100
    starts = rng.integers(0, len(genome) - L + 1, n)
    starts[:30] = np.arange(30) * 100            # every base is covered
    reads = np.stack([genome[s:s + L] for s in starts]).reshape(-1).copy()
    sub = np.nonzero(rng.random(len(reads)) < 0.02)[0]
    reads[sub] = random_reads(rng, len(sub))
    reads[rng.integers(0, len(reads), 5)] = ord("N")
    return reads, n, L


def _path_reads(k, n_keys):
    """one read of k + n_keys - 1 bases: a path of n_keys k-mers"""
    return random_reads(np.random.default_rng(4300 + 10 * k + n_keys), k + n_keys - 1), 1, k + n_keys - 1


def _low_bases_reads(k):
    """reads of all A behind four seeded bases.  Base 0 is the LOWEST two bits of a word, so every key is below 4^4 -- all keys share
    their top bits and one directory bin holds the whole table"""
    rng = np.random.default_rng(4400 + k)
    n, L = 40, k + 6
    reads = np.full((n, L), ord("A"), np.uint8)
    reads[:, :4] = random_reads(rng, 4 * n).reshape(n, 4)
    return reads.reshape(-1), n, L


class Table:
    """a count table on the device, its host copy and, made on first use and kept, its reference per (min_count, counts or not)"""

    def __init__(self, ctx, reads, n, L, k):
        self.k, self.ctx = k, ctx
        f = ctx.count_canonical if k <= 31 else ctx.count_canonical2
        self.d_k, self.d_c = f(ctx.to_device(reads), n, L, k)
        self.tk, self.tc = u64(self.d_k), u64(self.d_c)
        self.n = len(self.tc)
        self._ref = {}

    def ref(self, min_count=1, with_counts=True):
        key = (min_count, with_counts)
        if key not in self._ref:
            e, f, nb = graph_np.adjacency_np(self.tk, self.tc if with_counts else None, self.k, min_count)
            self._ref[key] = (e, f, nb, graph_np.unitig_ends_np(e, f, nb))
        return self._ref[key]

    def run(self, min_count=1, with_counts=True, flips=True, neighbors=True):
        f = self.ctx.count_adjacency if self.k <= 31 else self.ctx.count_adjacency2
        return f(self.d_k, self.d_c if with_counts else None, self.k, min_count, flips=flips, neighbors=neighbors)


_TABLES = {}


def _table(ctx, kind, k, *args):
    key = (kind.__name__, k) + args
    if key not in _TABLES or _TABLES[key].ctx is not ctx:
        _TABLES[key] = Table(ctx, *kind(k, *args), k)
    return _TABLES[key]


def _check(t, min_count=1, with_counts=True):
    """adjacency, edge histogram and unitig ends of one table against the reference; -> the reference"""
    ctx = t.ctx
    want_e, want_f, want_nb, want_ends = t.ref(min_count, with_counts)
    edges, flips, nbr = t.run(min_count, with_counts)
    assert np.array_equal(edges.cpu().numpy(), want_e), (t.k, t.n, "edges")
    assert np.array_equal(flips.cpu().numpy(), want_f), (t.k, t.n, "flips")
    assert nbr.shape == (t.n, 8) and np.array_equal(u64(nbr), want_nb), (t.k, t.n, "nbr")
    s = ctx.count_edge_histogram(edges)
    assert list(s.bins) == np.bincount(want_e, minlength=256).tolist()
    ends = ctx.count_unitig_ends(edges, flips, nbr)
    assert np.array_equal(ends.cpu().numpy(), want_ends), (t.k, t.n, "ends")
    return want_e, want_f, want_nb, want_ends


def _check_both_routes(t, min_count=1, with_counts=True):
    ref = _check(t, min_count, with_counts)
    try:
        t.ctx.set_work_buffer_limit(1)   # no directory fits: every search is a plain binary search, and nothing is refused
        _check(t, min_count, with_counts)
    finally:
        t.ctx.set_work_buffer_limit(0)
    return ref


# ---------------------------------------------------------------- dense and sparse graphs
@pytest.mark.parametrize("k", DENSE_KS)
def test_dense_graph(ctx, k):
    t = _table(ctx, _dense_reads, k)
    assert t.n > 0.5 * (4**k // 2)
    edges, flips, nbr, _ = _check_both_routes(t)
    nib = np.array([bin(v).count("1") for v in range(16)])
    assert (nib[edges & 15] == 4).any() and (nib[edges >> 4] == 4).any()   # a full group of four consecutive keys
    if k % 2 == 0:   # a palindrome is somebody's neighbour, and such an edge is never flipped
        lo, hi = graph_np.split(t.tk)
        rl, rh = graph_np.revcomp2(lo, hi, k)
        pal = np.nonzero((rl == lo) & (rh == hi))[0]
        assert len(pal) > 0
        to_pal = np.isin(nbr, pal.astype(np.uint64))
        assert to_pal.any()
        bits = (flips[:, None] >> np.arange(8, dtype=np.uint8)) & 1
        assert not bits[to_pal].any()


@pytest.mark.parametrize("k", SPARSE_KS)
def test_sparse_graph(ctx, k):
    t = _table(ctx, _sparse_reads, k)
    edges, flips, _, ends = _check_both_routes(t)
    s = ctx.count_edge_histogram(t.run(flips=False, neighbors=False))
    assert s.n_entries == t.n and s.n_interior > 0 and s.n_tips > 0 and s.n_branching > 0   # paths, tips and forks
    assert flips.any() and (edges & ~flips).any()
    want = graph_np.graph_summary_np(s.bins)
    assert (s.n_edges, s.n_isolated, s.n_tips, s.n_branching, s.n_interior) == tuple(
        want[f] for f in ("n_edges", "n_isolated", "n_tips", "n_branching", "n_interior"))
    assert np.array_equal(s.degrees, want["degrees"])
    assert (ends != 0).any() and (ends == 0).any()   # ends of unitigs and entries inside one


# ---------------------------------------------------------------- degenerate tables
@pytest.mark.parametrize("k", (15, 33))
def test_empty_table(ctx, k):
    import torch

    kmers = torch.zeros((0,) if k <= 31 else (0, 2), dtype=torch.int64, device=ctx.device)
    counts = torch.zeros(0, dtype=torch.int64, device=ctx.device)
    f = ctx.count_adjacency if k <= 31 else ctx.count_adjacency2
    edges, flips, nbr = f(kmers, counts, k, flips=True, neighbors=True)
    assert edges.numel() == 0 and flips.numel() == 0 and nbr.shape == (0, 8)
    assert ctx.count_unitig_ends(edges, flips, nbr).numel() == 0
    bins = torch.arange(256, dtype=torch.int64, device=ctx.device)
    assert list(ctx.count_edge_histogram(edges, out=bins).bins) == list(range(256))   # n == 0: the bins are left as they are


@pytest.mark.parametrize("k", (2, 15, 31, 33, 64))
def test_all_a_is_a_self_loop(ctx, k):
    t = Table(ctx, np.full(k + 3, ord("A"), np.uint8), 1, k + 3, k)
    assert t.n == 1 and not t.tk.any()
    edges, flips, nbr, ends = _check_both_routes(t)
    assert edges.tolist() == [0x11] and flips.tolist() == [0] and ends.tolist() == [3]
    assert [int(v) for v in nbr[0]] == [0, NO_ENTRY, NO_ENTRY, NO_ENTRY, 0, NO_ENTRY, NO_ENTRY, NO_ENTRY]


@pytest.mark.parametrize("k", (15, 33))
def test_a_lone_key(ctx, k):
    t = _table(ctx, _path_reads, k, 1)
    assert t.n == 1
    edges, _, nbr, ends = _check_both_routes(t)
    assert edges.tolist() == [0] and (nbr == NO_ENTRY).all() and ends.tolist() == [3]


@pytest.mark.parametrize("n_keys", range(2, 10))
@pytest.mark.parametrize("k", (15, 33))
def test_tables_at_and_below_one_line_of_keys(ctx, k, n_keys):
    t = _table(ctx, _path_reads, k, n_keys)
    assert t.n == n_keys
    edges, _, _, ends = _check_both_routes(t)
    assert int(np.unpackbits(edges).sum()) == 2 * (n_keys - 1)   # a path: every edge listed from both of its entries
    assert int(np.unpackbits(ends).sum()) == 2                   # one unitig


@pytest.mark.parametrize("k", (21, 47))
def test_one_directory_bin_holds_the_whole_table(ctx, k):
    t = _table(ctx, _low_bases_reads, k)
    lo, hi = graph_np.split(t.tk)
    assert t.n > 16 and not hi.any() and int(lo.max()) < 4**4
    edges, _, _, _ = _check_both_routes(t)
    assert edges.any()


# ---------------------------------------------------------------- presence
@pytest.mark.parametrize("k", (6, 21, 47))
def test_presence(ctx, k):
    t = _table(ctx, _dense_reads if k < 7 else _sparse_reads, k)
    assert (t.tc >= 2).any() and (t.tc < 2).any()
    full = _check_both_routes(t, 1)
    none = _check_both_routes(t, 1, with_counts=False)   # d_counts == NULL: every entry is present
    assert all(np.array_equal(a, b) for a, b in zip(full, none))
    e2, f2, nb2, _ = _check_both_routes(t, 2)
    keep = t.tc >= 2
    assert not e2[~keep].any() and (nb2[~keep] == NO_ENTRY).all()   # an absent entry has no edges ...
    gone = np.nonzero(~keep)[0].astype(np.uint64)
    assert not np.isin(nb2, gone).any()                             # ... and is nobody's neighbour
    assert e2.any() and (e2 != full[0]).any()
    top = int(t.tc.max()) + 1
    e0, f0, nb0, ends0 = _check_both_routes(t, top)                 # above every count: nothing is present
    assert not e0.any() and not f0.any() and (nb0 == NO_ENTRY).all() and (ends0 == 3).all()
    # the same graph from the filtered table, after index translation
    fk, fc = (ctx.count_filter if k <= 31 else ctx.count_filter2)(t.d_k, t.d_c, 2)
    f = ctx.count_adjacency if k <= 31 else ctx.count_adjacency2
    ef, ff, nbf = f(fk, fc, k, 1, flips=True, neighbors=True)
    assert np.array_equal(ef.cpu().numpy(), e2[keep]) and np.array_equal(ff.cpu().numpy(), f2[keep])
    new_index = (np.cumsum(keep) - 1).astype(np.uint64)
    sub = nb2[keep]
    moved = np.where(sub == NO_ENTRY, np.uint64(NO_ENTRY), new_index[np.where(sub == NO_ENTRY, 0, sub).astype(np.int64)])
    assert np.array_equal(u64(nbf), moved)


# ---------------------------------------------------------------- output selection
@pytest.mark.parametrize("k", (6, 31, 64))
def test_every_combination_of_outputs(ctx, k):
    t = _table(ctx, _dense_reads if k < 7 else _sparse_reads, k)
    want_e, want_f, want_nb, _ = t.ref()
    for limit in (0, 1):
        try:
            ctx.set_work_buffer_limit(limit)
            edges = t.run(flips=False, neighbors=False)
            assert np.array_equal(edges.cpu().numpy(), want_e)
            edges, flips = t.run(flips=True, neighbors=False)
            assert np.array_equal(edges.cpu().numpy(), want_e) and np.array_equal(flips.cpu().numpy(), want_f)
            edges, nbr = t.run(flips=False, neighbors=True)
            assert np.array_equal(edges.cpu().numpy(), want_e) and np.array_equal(u64(nbr), want_nb)
        finally:
            ctx.set_work_buffer_limit(0)


# ---------------------------------------------------------------- edge histogram and unitig ends on their own
@pytest.mark.parametrize("n,offset", [(1, 0), (15, 0), (16, 0), (4096, 0), (4097, 3), (70001, 0), (70001, 5), (33, 15)])
def test_edge_histogram(ctx, n, offset):
    """sizes that are no multiple of a lane's 16 bytes or of a block's 4096, and arrays that do not start 16-byte aligned"""
    import torch

    rng = np.random.default_rng(4500 + n + offset)
    host = rng.integers(0, 256, n + offset).astype(np.uint8)
    host[: (n + offset) // 2] = 0x11          # one hot bin, as in a real graph
    dev = ctx.to_device(host)[offset:]
    want = np.bincount(host[offset:], minlength=256)
    assert list(ctx.count_edge_histogram(dev).bins) == want.tolist()
    before = rng.integers(0, 2**62, 256)
    bins = torch.from_numpy(before.copy()).to(ctx.device)
    s = ctx.count_edge_histogram(dev, out=bins)   # accumulated into bins that are not zero
    assert list(s.bins) == (before + want).tolist() and bins.cpu().numpy().tolist() == list(s.bins)


def test_unitig_ends_with_indices_outside_the_table(ctx):
    edges = np.array([0x11, 0x11], np.uint8)
    flips = np.zeros(2, np.uint8)
    nbr = np.full((2, 8), NO_ENTRY, np.uint64)
    nbr[0, 0], nbr[0, 4] = 1, 7          # slot 4 names an entry that does not exist: that side ends, nothing is read
    nbr[1, 4], nbr[1, 0] = 0, 2**40
    want = graph_np.unitig_ends_np(edges, flips, nbr)
    assert want.tolist() == [2, 1]
    got = ctx.count_unitig_ends(ctx.to_device(edges), ctx.to_device(flips), ctx.to_device(nbr))
    assert got.cpu().numpy().tolist() == want.tolist()


# ---------------------------------------------------------------- argument errors
def test_argument_errors(ctx):
    import torch

    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    lib = ctx.lib
    keys = torch.zeros(2 * 8 + 1, dtype=torch.int64, device=ctx.device)
    edges = torch.zeros(8, dtype=torch.uint8, device=ctx.device)
    one, two = lib.kmx_count_adjacency, lib.kmx_count_adjacency2
    for k in (0, 1, 32, 33, 64):
        assert one(ctx._h, _ptr(keys), None, 8, k, 1, _ptr(edges), None, None) == _lib.E_K_RANGE, k
    for k in (1, 2, 31, 32, 65):
        assert two(ctx._h, _ptr(keys), None, 8, k, 1, _ptr(edges), None, None) == _lib.E_K_RANGE, k
    assert one(ctx._h, _ptr(keys), None, 8, 31, 1, None, None, None) == _lib.E_ARG
    assert two(ctx._h, _ptr(keys), None, 8, 33, 1, None, None, None) == _lib.E_ARG
    assert one(ctx._h, None, None, 8, 31, 1, _ptr(edges), None, None) == _lib.E_ARG
    assert two(ctx._h, C.c_void_p(keys.data_ptr() + 8), None, 8, 33, 1, _ptr(edges), None, None) == _lib.E_ARG   # not 16-byte aligned
    assert one(None, _ptr(keys), None, 8, 31, 1, _ptr(edges), None, None) == _lib.E_ARG
    assert one(ctx._h, _ptr(keys), None, 2**40 + 1, 31, 1, _ptr(edges), None, None) == _lib.E_ARG
    assert one(ctx._h, None, None, 0, 31, 1, None, None, None) == _lib.OK   # n == 0: a no-op
    assert lib.kmx_count_edge_histogram(ctx._h, _ptr(edges), 8, None) == _lib.E_ARG
    assert lib.kmx_count_edge_histogram(ctx._h, None, 8, _ptr(keys)) == _lib.E_ARG
    assert lib.kmx_count_unitig_ends(ctx._h, _ptr(edges), None, _ptr(keys), 2, _ptr(edges)) == _lib.E_ARG
    assert lib.kmx_count_unitig_ends(ctx._h, _ptr(edges), _ptr(edges), _ptr(keys), 2, None) == _lib.E_ARG
    ctx.synchronize()
    assert not edges.any()   # nothing ran
