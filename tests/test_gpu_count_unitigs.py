"""The unitigs of a count table's de Bruijn graph on the GPU: kmx_count_unitigs(2) and kmx_count_unitig_sequences(2)
(kmx_count_unitigs.hip).

Everything is exact: nodes, offsets, circular flags, count sums and sequences are compared element by element with the host reference
tests/unitig_np.py (sequential walking straight from the definitions, pinned against brute force over strings in
tests/test_unitig_np.py).  The tables are what Context.count_canonical(2) makes of seeded reads, as in tests/test_gpu_count_graph.py; a
circular sequence is a read with its first k - 1 bases appended.  A table, its adjacency and its reference are made once per module
and shared.  Every family asserts on the reference that it holds what it is there for."""
import ctypes as C

import numpy as np
import pytest

from tests import graph_np, unitig_np
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import random_reads, u64
from tests.test_gpu_count_graph import _dense_reads, _path_reads, _sparse_reads

pytestmark = pytest.mark.gpu

SPARSE_KS = (15, 21, 31, 33, 47, 63, 64)
HAIRPINS = {6: "GGTTACGTAACC", 8: "CCAGTACGTACTGG"}


# ---------------------------------------------------------------- the read batches
def _ragged(seqs):
    """sequences of different lengths as one batch: (bases, offsets)"""
    offsets = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
    return np.concatenate(seqs).astype(np.uint8), offsets


def _circle(rng, m, k):
    """a circular sequence of m bases as a read: m k-mers, the last k - 1 of them across the seam"""
    s = random_reads(rng, m)
    return np.concatenate([s, s[:k - 1]])


def _circles_reads(k):
    """circular sequences of 2 (the AC repeat), 3, 64, 1000 and 1024 nodes beside linear reads"""
    rng = np.random.default_rng(6100 + k)
    ac = np.frombuffer(b"AC" * ((k + 3) // 2 + 1), np.uint8)[:k + 1]
    acg = np.frombuffer(b"ACG" * (k // 3 + 2), np.uint8)[:k + 2]
    seqs = [ac, acg] + [_circle(rng, m, k) for m in (64, 1000, 1024)] + [random_reads(rng, k + 200), random_reads(rng, k + 7)]
    return _ragged(seqs)


def _dense8_reads(k):
    """2048 reads of 60 bases: three windows per canonical 8-mer"""
    return random_reads(np.random.default_rng(6200 + k), 2048 * 60), 2048, 60


def _hairpin_reads(k):
    h = np.frombuffer(HAIRPINS[k].encode(), np.uint8)
    return h, 1, len(h)


class Table:
    """a count table on the device with its host copy; adjacency and reference per (min_count, counts or not), made on first use"""

    def __init__(self, ctx, k, reads, n=None, L=None, offsets=None):
        self.k, self.ctx = k, ctx
        f = ctx.count_canonical if k <= 31 else ctx.count_canonical2
        if offsets is None:
            self.d_k, self.d_c = f(ctx.to_device(reads), n, L, k)
        else:
            self.d_k, self.d_c = f(ctx.to_device(reads), len(offsets) - 1, 0, k, offsets=ctx.to_device(offsets))
        self.tk, self.tc = u64(self.d_k), u64(self.d_c)
        self.n = len(self.tc)
        self._ref, self._adj = {}, {}

    def adjacency(self, min_count=1, with_counts=True):
        key = (min_count, with_counts)
        if key not in self._adj:
            f = self.ctx.count_adjacency if self.k <= 31 else self.ctx.count_adjacency2
            self._adj[key] = f(self.d_k, self.d_c if with_counts else None, self.k, min_count, flips=True, neighbors=True)
        return self._adj[key]

    def ref(self, min_count=1, with_counts=True):
        key = (min_count, with_counts)
        if key not in self._ref:
            tc = self.tc if with_counts else None
            e, f, nb = graph_np.adjacency_np(self.tk, tc, self.k, min_count)
            out = unitig_np.unitigs_np(self.tk, tc, self.k, min_count, e, f, nb)
            self._ref[key] = out + (unitig_np.sequences_np(self.tk, self.k, out[0], out[1]),)
        return self._ref[key]

    def run(self, min_count=1, with_counts=True, adjacency=True):
        f = self.ctx.count_unitigs if self.k <= 31 else self.ctx.count_unitigs2
        return f(self.d_k, self.d_c if with_counts else None, self.k, min_count,
                 adjacency=self.adjacency(min_count, with_counts) if adjacency else None)


_TABLES = {}


def _table(ctx, kind, k):
    key = (kind.__name__, k)
    if key not in _TABLES or _TABLES[key].ctx is not ctx:
        made = kind(k)
        _TABLES[key] = Table(ctx, k, made[0], offsets=made[1]) if len(made) == 2 else Table(ctx, k, *made)
    return _TABLES[key]


def _same(got, want, what):
    nodes, offsets, circular, sums, seq = want
    assert got.n_unitigs == len(circular), (what, got.n_unitigs, len(circular))
    assert np.array_equal(u64(got.offsets), offsets), (what, "offsets")
    assert np.array_equal(u64(got.nodes), nodes), (what, "nodes")
    assert np.array_equal(got.circular.cpu().numpy(), circular), (what, "circular")
    assert np.array_equal(u64(got.count_sums), sums), (what, "count_sums")
    assert np.array_equal(got.sequences().cpu().numpy(), seq), (what, "sequences")
    assert np.array_equal(got.lengths.cpu().numpy(), np.diff(offsets.astype(np.int64)))


def _check(t, min_count=1, with_counts=True, adjacency=True):
    want = t.ref(min_count, with_counts)
    got = t.run(min_count, with_counts, adjacency)
    _same(got, want, (t.k, t.n, min_count, with_counts))
    return want, got


def _lengths(want):
    return np.diff(want[1].astype(np.int64))


# ---------------------------------------------------------------- 1. overlapping reads with substitutions
@pytest.mark.parametrize("with_counts", (True, False))
@pytest.mark.parametrize("min_count", (1, 2))
@pytest.mark.parametrize("k", SPARSE_KS)
def test_sparse_graph(ctx, k, min_count, with_counts):
    t = _table(ctx, _sparse_reads, k)
    want, got = _check(t, min_count, with_counts)
    lens = _lengths(want)
    assert len(lens) > 10 and (want[0] & np.uint64(1)).any() and not (want[0] & np.uint64(1)).all()   # both orientations
    if with_counts and min_count == 2:   # the substitutions are gone: long unitigs (k = 64 leaves 37 windows per read: shorter ones)
        assert (t.tc < 2).any() and int(want[1][-1]) == int((t.tc >= 2).sum()) < t.n   # entries that are not present are in no unitig
        assert lens.max() > (64 if k < 64 else 32)
    else:                                # tips and bubbles: short unitigs beside single nodes
        assert int(want[1][-1]) == t.n and lens.max() > 32 and (lens == 1).any()
    u = int(np.argmax(lens))
    assert got.sequence(u) == bytes(want[4][int(want[1][u]) + u * (k - 1):int(want[1][u + 1]) + (u + 1) * (k - 1)])


@pytest.mark.parametrize("k", (21, 47))
def test_the_adjacency_is_made_when_it_is_not_given(ctx, k):
    t = _table(ctx, _sparse_reads, k)
    _check(t, 2, True, adjacency=False)


# ---------------------------------------------------------------- 2. one long path
@pytest.mark.parametrize("k", (21, 47))
def test_one_path_of_5000(ctx, k):
    t = _path_table(ctx, k)
    want, _ = _check(t)
    assert t.n == 5000 and _lengths(want).tolist() == [5000] and want[2].tolist() == [0]   # one linear unitig: 14 rounds, 40 blocks
    _check(t, 1, False)


def _path_table(ctx, k):
    key = ("path5000", k)
    if key not in _TABLES or _TABLES[key].ctx is not ctx:
        _TABLES[key] = Table(ctx, k, *_path_reads(k, 5000))
    return _TABLES[key]


# ---------------------------------------------------------------- 3. cycles
@pytest.mark.parametrize("k", (15, 31, 33, 47))
def test_circular_sequences(ctx, k):
    t = _table(ctx, _circles_reads, k)
    want, _ = _check(t)
    lens, circ = _lengths(want), want[2]
    assert sorted(lens[circ == 1].tolist()) == [2, 3, 64, 1000, 1024]      # powers of two and others
    assert (circ == 0).any() and lens[circ == 0].max() > 64
    _check(t, 1, False)
    _check(t, 2)   # every count is 1: nothing is present
    assert t.ref(2)[1].tolist() == [0]


# ---------------------------------------------------------------- 4. dense graphs, palindromes, hairpins
@pytest.mark.parametrize("k", (4, 5, 6, 8))
def test_dense_graph(ctx, k):
    t = _table(ctx, _dense_reads if k < 8 else _dense8_reads, k)
    for min_count, with_counts in ((1, True), (2, True), (1, False)):
        want, _ = _check(t, min_count, with_counts)
        lens = _lengths(want)
        assert (lens == 1).sum() > 0.8 * len(lens) and int(want[1][-1]) > 100   # nearly all single nodes
    pal = unitig_np.palindromes_np(t.tk, k)
    assert pal.any() == (k % 2 == 0)
    if k % 2 == 0:   # a palindrome is a unitig of its own, read forward
        want = t.ref()
        first = want[0][want[1][:-1].astype(np.int64)]
        assert np.isin(2 * np.nonzero(pal)[0].astype(np.uint64), first[_lengths(want) == 1]).all()


@pytest.mark.parametrize("k", (6, 8))
def test_hairpins(ctx, k):
    t = _table(ctx, _hairpin_reads, k)
    want, _ = _check(t)
    pal = np.nonzero(unitig_np.palindromes_np(t.tk, k))[0]
    assert len(pal) == 1 and sorted(_lengths(want).tolist()) == [1, t.n - 1]   # y .. -> palindrome -> .. rc(y): two unitigs
    _check(t, 1, False)


# ---------------------------------------------------------------- 5. edge cases
@pytest.mark.parametrize("k", (15, 33))
def test_empty_table(ctx, k):
    import torch

    kmers = torch.zeros((0,) if k <= 31 else (0, 2), dtype=torch.int64, device=ctx.device)
    counts = torch.zeros(0, dtype=torch.int64, device=ctx.device)
    got = (ctx.count_unitigs if k <= 31 else ctx.count_unitigs2)(kmers, counts, k)
    assert got.n_unitigs == 0 and got.nodes.numel() == 0 and got.offsets.cpu().tolist() == [0]
    assert got.sequences().numel() == 0 and got.lengths.numel() == 0


@pytest.mark.parametrize("k", (2, 15, 31, 33, 64))
def test_one_entry(ctx, k):
    t = Table(ctx, k, np.full(k + 3, ord("A"), np.uint8), 1, k + 3)
    assert t.n == 1
    want, got = _check(t)
    assert want[0].tolist() == [0] and want[1].tolist() == [0, 1] and want[2].tolist() == [0] and want[3].tolist() == [4]
    assert got.sequence(0) == b"A" * k
    _check(t, 5)   # not present: no unitig


@pytest.mark.parametrize("k", (21, 47))
def test_optional_outputs_null(ctx, k):
    import torch

    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    t = _table(ctx, _sparse_reads, k)
    want = t.ref(2)
    edges, flips, nbr = t.adjacency(2)
    fn = ctx.lib.kmx_count_unitigs if k <= 31 else ctx.lib.kmx_count_unitigs2
    nodes = torch.zeros(t.n, dtype=torch.int64, device=ctx.device)
    offsets = torch.zeros(t.n + 1, dtype=torch.int64, device=ctx.device)
    circular = torch.full((t.n,), 7, dtype=torch.uint8, device=ctx.device)
    nu, nn = C.c_uint64(0), C.c_uint64(0)
    for circ in (None, circular):
        st = fn(ctx._h, _ptr(t.d_k), _ptr(t.d_c), t.n, k, 2, _ptr(edges), _ptr(flips), _ptr(nbr), _ptr(nodes), _ptr(offsets),
                _ptr(circ) if circ is not None else None, None, C.byref(nu), C.byref(nn))
        assert st == _lib.OK
        assert (nu.value, nn.value) == (len(want[2]), len(want[0]))
        assert np.array_equal(u64(nodes)[:nn.value], want[0]) and np.array_equal(u64(offsets)[:nu.value + 1], want[1])
    assert np.array_equal(circular.cpu().numpy()[:nu.value], want[2]) and (circular.cpu().numpy()[nu.value:] == 7).all()


def test_work_buffer_cap(ctx):
    from kmers_amd import _lib

    t = _table(ctx, _sparse_reads, 31)
    t.adjacency(2)
    try:
        ctx.set_work_buffer_limit(32 * t.n)   # the call needs a little more than 64 bytes per entry
        with pytest.raises(_lib.KmxError) as err:
            t.run(2)
        assert err.value.status == _lib.E_NOMEM
    finally:
        ctx.set_work_buffer_limit(0)
    _check(t, 2)


def test_argument_errors(ctx):
    import torch

    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    lib = ctx.lib
    keys = torch.zeros(2 * 8 + 1, dtype=torch.int64, device=ctx.device)
    by = torch.zeros(8, dtype=torch.uint8, device=ctx.device)
    out = torch.zeros(9, dtype=torch.int64, device=ctx.device)
    nbr = torch.full((64,), -1, dtype=torch.int64, device=ctx.device)
    nu, nn = C.c_uint64(9), C.c_uint64(9)
    one, two = lib.kmx_count_unitigs, lib.kmx_count_unitigs2

    def call(fn, k, kmers=keys, edges=by, flips=by, nb=nbr, nodes=out, offsets=out, h=(nu, nn), n=8, handle=None):
        p = lambda x: _ptr(x) if x is not None else None   # noqa: E731
        return fn(ctx._h if handle is None else handle, kmers if isinstance(kmers, C.c_void_p) else p(kmers), None, n, k, 1, p(edges), p(flips), p(nb),
                  p(nodes), p(offsets), None, None, C.byref(h[0]) if h else None, C.byref(h[1]) if h else None)

    for k in (0, 1, 32, 33, 64):
        assert call(one, k) == _lib.E_K_RANGE, k
    for k in (1, 2, 31, 32, 65):
        assert call(two, k) == _lib.E_K_RANGE, k
    for missing in ("edges", "flips", "nb", "nodes", "offsets"):
        assert call(one, 31, **{missing: None}) == _lib.E_ARG, missing
    assert call(one, 30, kmers=None) == _lib.E_ARG          # even k reads the keys
    assert call(one, 31, h=None) == _lib.E_ARG
    assert call(two, 33, kmers=C.c_void_p(keys.data_ptr() + 8)) == _lib.E_ARG   # not 16-byte aligned
    assert call(one, 31, n=2**40 + 1) == _lib.E_ARG
    assert call(one, 31, kmers=None, edges=None, flips=None, nb=None, nodes=None, offsets=None, n=0) == _lib.OK
    assert (nu.value, nn.value) == (0, 0)                    # n == 0: a no-op with both counts 0
    seq = lib.kmx_count_unitig_sequences
    assert seq(ctx._h, _ptr(keys), 8, 32, _ptr(out), _ptr(out), 1, _ptr(by)) == _lib.E_K_RANGE
    assert seq(ctx._h, _ptr(keys), 8, 31, None, _ptr(out), 1, _ptr(by)) == _lib.E_ARG
    assert seq(ctx._h, _ptr(keys), 8, 31, _ptr(out), _ptr(out), 9, _ptr(by)) == _lib.E_ARG   # more unitigs than entries
    assert seq(ctx._h, None, 8, 31, None, None, 0, None) == _lib.OK
    ctx.synchronize()
    assert not out.any() and not by.any()   # nothing ran


# ---------------------------------------------------------------- 6. inconsistent inputs
def _garbage(rng, n):
    """random bytes and random u64, most indices inside the table or just past it; over a third of the entries a random tour whose
    consecutive entries name each other with one edge on the facing sides, so that links do occur -- and the rest disturbs them"""
    edges, flips = rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 256, n).astype(np.uint8)
    nbr = rng.integers(0, 2**64, (n, 8), dtype=np.uint64)
    near = rng.random((n, 8)) < 0.7
    nbr[near] = rng.integers(0, n + n // 8, int(near.sum())).astype(np.uint64)
    tour = rng.permutation(n)[: n // 3]
    a, b = tour[:-1], tour[1:]
    ca, cb = rng.integers(0, 4, len(a)), rng.integers(0, 4, len(a))
    edges[a] = (edges[a] & 0xF0) | (1 << ca).astype(np.uint8)
    edges[b] = (edges[b] & 0x0F) | (16 << cb).astype(np.uint8)
    nbr[a, ca], nbr[b, 4 + cb] = b.astype(np.uint64), a.astype(np.uint64)
    flips[tour] = 0
    return edges, flips, nbr


@pytest.mark.parametrize("k,n", [(31, 1000), (47, 70001)])
def test_garbage_adjacency(ctx, k, n):
    """any bytes in d_edges / d_flips / d_nbr: the call succeeds and answers as the reference does on the same garbage (every index is
    checked against n before it is used, and only mutual links count)"""
    rng = np.random.default_rng(6300 + k)
    edges, flips, nbr = _garbage(rng, n)
    counts = rng.integers(0, 4, n).astype(np.uint64)
    words = 1 if k <= 31 else 2
    keys = rng.integers(0, 2**62, (n, words), dtype=np.uint64).reshape(n if words == 1 else (n, 2))   # (odd k: never read)
    want = unitig_np.unitigs_np(None, counts, k, 2, edges, flips, nbr)
    lens = np.diff(want[1].astype(np.int64))
    assert lens.max() > 2 and int(want[1][-1]) == int((counts >= 2).sum()) < n
    f = ctx.count_unitigs if k <= 31 else ctx.count_unitigs2
    got = f(ctx.to_device(keys), ctx.to_device(counts), k, 2, adjacency=(ctx.to_device(edges), ctx.to_device(flips), ctx.to_device(nbr)))
    assert got.n_unitigs == len(want[2])
    assert np.array_equal(u64(got.offsets), want[1]) and np.array_equal(u64(got.nodes), want[0])
    assert np.array_equal(got.circular.cpu().numpy(), want[2]) and np.array_equal(u64(got.count_sums), want[3])
