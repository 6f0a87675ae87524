"""The connected components of the unitig graph on the GPU: kmx_count_unitig_components (kmx_count_components.hip) and what the Python
layer builds on it (Context.count_unitig_components, UnitigComponents.keep, ReadPaths.components,
Context.count_drop_small_components(2)).

Every comparison is u64 equality of whole arrays -- labels, ids, records, the count -- with the sequential host reference
tests/component_np.py (pinned against hand-written graphs, a breadth-first search and scipy in tests/test_component_np.py), over
poisoned output buffers with guard words behind them.  The call reads indices only, so most graphs here are link arrays built on
the host; the real ones come through tests/test_gpu_unitig_links.Linked, the string cases are tests/test_clean_np.py's, the dense
tables tests/test_gpu_count_unitigs.py's.  Every family asserts of its own input that it holds what it is there for."""
import ctypes as C

import numpy as np
import pytest

from tests import component_np
from tests.component_np import NONE, both_ways, components_np, link_arrays
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import random_reads, u64
from tests.test_clean_np import cases, key_list, table
from tests.test_component_np import CHAIN, chain_orders, chain_pairs, fork_cases, random_graph, round_cap
from tests.test_gpu_count_graph import _dense_reads
from tests.test_gpu_count_unitigs import _dense8_reads, _table
from tests.test_gpu_unitig_clean import _count
from tests.test_gpu_unitig_links import Linked

pytestmark = pytest.mark.gpu

POISON = -0x5A5A5A5A5A5A5A5B
E_ARG, E_NOMEM = 1, 6
GUARD = 32


def dev(ctx, a):
    import torch

    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(ctx.device)


class Graph:
    """link arrays (and optionally unitig offsets, sums, a mask) on the host and on the device"""

    def __init__(self, ctx, U, lo, tg, offsets=None, sums=None, mask=None):
        self.ctx, self.U, self.lo, self.tg, self.offsets, self.sums, self.mask = ctx, U, lo, tg, offsets, sums, mask
        self.d = {name: dev(ctx, a) for name, a in (("lo", lo), ("tg", tg if len(tg) else None), ("offsets", offsets), ("sums", sums), ("mask", mask))}
        self._want = None

    def want(self):
        if self._want is None:
            self._want = components_np(self.offsets, self.sums, self.lo, self.tg, self.mask, U=self.U)
        return self._want


def raw(g, ids=True, records=True, max_components=None, rounds=True, handle="ctx", h_n=True, n_unitigs=None, n_links=None, **override):
    """the C call as it is, over poisoned buffers with GUARD words behind them -> (status, labels, ids, records, C, rounds), the
    three arrays as u64 on the host, guards and all (None where not asked for)"""
    import torch

    from kmers_amd.api import _ptr

    ctx = g.ctx
    U = g.U if n_unitigs is None else n_unitigs
    room = (g.want()[3] if max_components is None else max_components) if records else 0
    fresh = lambda n: torch.full((n + GUARD,), POISON, dtype=torch.int64, device=ctx.device)
    d_labels, d_ids, d_rec = fresh(g.U), fresh(g.U) if ids else None, fresh(4 * room) if records else None
    a = {**g.d, "labels": d_labels, **override}
    c, r = C.c_uint64(2**64 - 1), C.c_uint32(2**32 - 1)
    st = ctx.lib.kmx_count_unitig_components(ctx._h if handle == "ctx" else handle, _ptr(a["offsets"]), _ptr(a["sums"]), U, _ptr(a["lo"]), _ptr(a["tg"]),
                                             len(g.tg) if n_links is None else n_links, _ptr(a["mask"]), _ptr(a["labels"]), _ptr(d_ids), _ptr(d_rec), room,
                                             C.byref(c) if h_n else None, C.byref(r) if rounds else None)
    ctx.synchronize()
    host = lambda t: None if t is None else u64(t)
    return st, host(d_labels), host(d_ids), host(d_rec), c.value, r.value if rounds else None


def guards_intact(*sized):
    return all(a is None or (a[n:] == np.uint64(POISON & (2**64 - 1))).all() for a, n in sized)


def check(g, **kw):
    """one call against the reference: every word, the count, nothing behind the arrays -> (C, rounds)"""
    labels, ids, rec, n = g.want()
    st, got_l, got_i, got_r, got_n, rounds = raw(g, **kw)
    assert st == 0 and got_n == n, (st, got_n, n)
    assert np.array_equal(got_l[:g.U], labels), "labels"
    assert got_i is None or np.array_equal(got_i[:g.U], ids), "ids"
    assert got_r is None or np.array_equal(got_r[:4 * n].reshape(-1, 4), rec), "records"
    assert guards_intact((got_l, g.U), (got_i, g.U), (got_r, 4 * n))
    return n, rounds


def weights(rng, U):
    """unitig offsets and count sums to go with synthetic links: lengths 1 .. 39, sums over the whole u64 range (they wrap)"""
    return np.concatenate([[0], np.cumsum(rng.integers(1, 40, U))]).astype(np.uint64), rng.integers(0, 2**64, U, dtype=np.uint64)


# ---------------------------------------------------------------- synthetic link arrays
@pytest.mark.parametrize("U", (0, 1, 2, 63, 64, 65, 4097))
def test_small_sizes(ctx, U):
    """around a wave, around a scanned range of 4096; pairs joined two and two, the rest alone"""
    rng = np.random.default_rng(5000 + U)
    pairs = [(u, u + 1) for u in range(0, U - 1, 3)] + ([(0, U - 1)] if U > 2 else [])
    offsets, sums = weights(rng, U)
    g = Graph(ctx, U, *link_arrays(U, both_ways(pairs)), offsets, sums)
    n, rounds = check(g)
    assert (rounds == 0) if U == 0 else (1 <= rounds <= round_cap(max(U, 2)))
    assert n == U - len(pairs)                                               # (the pairs close no cycle: each joins two components)


_CHAINS = {}


def _chain(ctx, name):
    if name not in _CHAINS or _CHAINS[name].ctx is not ctx:
        rng = np.random.default_rng(5100)
        _CHAINS[name] = Graph(ctx, CHAIN, *link_arrays(CHAIN, both_ways(chain_pairs(chain_orders()[name]))), *weights(rng, CHAIN))
    return _CHAINS[name]


@pytest.mark.parametrize("name", ("index order", "reverse order", "permuted"))
def test_long_chain(ctx, name):
    """2^16 unitigs in a row: one component, and a number of rounds that only doubling reaches (the cap separates it from a walk of
    the chain, which needs about U; the synchronous model of tests/component_np.py takes 17, 17 and 15)"""
    g = _chain(ctx, name)
    n, rounds = check(g)
    assert n == 1 and g.want()[2][0, 1] == CHAIN
    assert rounds <= round_cap(CHAIN), rounds


def test_star_with_the_largest_index_at_the_centre(ctx):
    """degree 8, four links on each side, and every hook aims at the centre's word"""
    U = 9
    lo, tg = link_arrays(U, both_ways([(8, v) for v in range(8)]))
    assert np.diff(lo.astype(np.int64))[16:18].tolist() == [4, 4]
    g = Graph(ctx, U, lo, tg, *weights(np.random.default_rng(5200), U))
    assert check(g)[0] == 1
    stars = 500                                                              # many of them, centres last: 8 leaves each
    pairs = [(8 * stars + s, 8 * s + j) for s in range(stars) for j in range(8)]
    g = Graph(ctx, 9 * stars, *link_arrays(9 * stars, both_ways(pairs)), *weights(np.random.default_rng(5201), 9 * stars))
    assert check(g)[0] == stars


_SPARSE = {}


def _sparse(ctx, one_way):
    """10^5 unitigs, about 0.6 links per unitig: many components of mixed size"""
    if one_way not in _SPARSE or _SPARSE[one_way].ctx is not ctx:
        rng = np.random.default_rng(5300)
        U = 100_000
        if one_way:
            lo, tg = random_graph(rng, U, 0.6)
        else:
            lo, tg = link_arrays(U, both_ways([(u, v) for u, v in rng.integers(0, U, (int(0.3 * U), 2)).tolist()]))
        _SPARSE[one_way] = Graph(ctx, U, lo, tg, *weights(rng, U))
    return _SPARSE[one_way]


@pytest.mark.parametrize("one_way", (False, True), ids=("both directions", "one direction only"))
def test_random_sparse_graph(ctx, one_way):
    g = _sparse(ctx, one_way)
    n, rounds = check(g)
    sizes = g.want()[2][:, 1]
    assert n > 30_000 and int((sizes == 1).sum()) > 10_000 and sizes.max() >= 8 and len(set(sizes.tolist())) >= 6
    assert rounds <= round_cap(g.U)


def test_isolated_unitigs_past_one_sweep_of_the_grid(ctx):
    """The launchers cap their grids at 1024 blocks of 256 lanes: 3 x 10^5 unitigs without a link are more than one sweep, and as
    many components as unitigs -- every range of the scan is full."""
    U = 300_000
    assert U > 1024 * 256
    rng = np.random.default_rng(5400)
    offsets, sums = weights(rng, U)
    labels = ids = np.arange(U, dtype=np.uint64)
    g = Graph(ctx, U, np.zeros(2 * U + 1, np.uint64), np.zeros(0, np.uint64), offsets, sums)
    m = np.diff(offsets.astype(np.int64)).astype(np.uint64)
    g._want = (labels, ids, np.stack([labels, np.ones(U, np.uint64), m, sums], 1), U)   # (the rule, read off: everything is its own root)
    assert check(g) == (U, 1)
    small = Graph(ctx, 1000, np.zeros(2001, np.uint64), np.zeros(0, np.uint64), offsets[:1001], sums[:1000])
    assert np.array_equal(small.want()[2], g._want[2][:1000])               # ... and the reference agrees with that reading


# ---------------------------------------------------------------- masks
@pytest.mark.parametrize("mask", ("ones", "zeros", "random", "cut"))
def test_masks(ctx, mask):
    base = _chain(ctx, "permuted") if mask == "cut" else _sparse(ctx, False)
    rng = np.random.default_rng(5500)
    U = base.U
    if mask == "cut":                                                        # the unitig in the middle of the chain
        order = chain_orders()["permuted"]
        m = np.ones(U, np.uint8)
        m[order[U // 2]] = 0
    else:
        m = {"ones": np.full(U, 255, np.uint8), "zeros": np.zeros(U, np.uint8), "random": (rng.integers(1, 256, U) * (rng.random(U) < 0.7)).astype(np.uint8)}[mask]
    g = Graph(ctx, U, base.lo, base.tg, base.offsets, base.sums, m)
    n, rounds = check(g)
    if mask == "ones":
        assert np.array_equal(g.want()[0], base.want()[0])
    if mask == "zeros":
        assert n == 0 and (g.want()[0] == NONE).all() and rounds == 1
    if mask == "random":
        assert n > base.want()[3] // 2 and (g.want()[0] == NONE).sum() > U // 5
    if mask == "cut":
        assert n == 2 and sorted(g.want()[2][:, 1].tolist()) == [U // 2 - 1, U // 2] and rounds <= round_cap(U)


# ---------------------------------------------------------------- arbitrary bytes
@pytest.mark.parametrize("U", (300, 20_001))
def test_inconsistent_inputs(ctx, U):
    """random words in the link offsets, the targets and the unitig offsets, exactly sized arrays: include/kmx.h defines the result,
    every index is checked before it is used, nothing behind the outputs is written"""
    rng = np.random.default_rng(5600 + U)
    n_links = 3 * U
    lo = np.minimum(np.concatenate([[0], np.cumsum(rng.integers(0, 4, 2 * U))]), n_links).astype(np.uint64)
    wild = rng.random(2 * U + 1) < 0.05
    lo[wild] = rng.integers(0, 2**64, int(wild.sum()), dtype=np.uint64)
    near = wild & (rng.random(2 * U + 1) < 0.5)
    lo[near] = rng.integers(0, n_links + 9, int(near.sum())).astype(np.uint64)   # descending, beyond the array, more than four
    tg = rng.integers(0, 2 * U, n_links).astype(np.uint64)
    wild = rng.random(n_links) < 0.03
    tg[wild] = rng.integers(0, 2**64, int(wild.sum()), dtype=np.uint64)
    tg[wild & (rng.random(n_links) < 0.5)] = np.uint64(2 * U)                # the first word that names no oriented unitig
    offsets, sums = weights(rng, U)
    wild = rng.random(U + 1) < 0.05
    offsets[wild] = rng.integers(0, 2**64, int(wild.sum()), dtype=np.uint64)
    lists = component_np.valid_lists(lo, tg, U)
    widths = [int(b) - int(a) for a, b in zip(lo[:-1], lo[1:])]
    assert any(w < 0 for w in widths) and any(w > 4 for w in widths) and (tg >= 2 * U).any()
    assert any(int(b) < int(a) for a, b in zip(offsets[:-1], offsets[1:]))
    assert 0 < sum(1 for l in lists if l) < 2 * U
    for mask in (None, (rng.random(U) < 0.9).astype(np.uint8)):
        g = Graph(ctx, U, lo, tg, offsets, sums, mask)
        n, _ = check(g)
        assert 1 < n < U
    # far fewer links than the offsets speak of: every list that reaches past n_links is empty
    g = Graph(ctx, U, lo, tg[:U], offsets, sums)
    check(g)


# ---------------------------------------------------------------- optional arguments, room, determinism
def test_optional_arguments(ctx):
    g = _sparse(ctx, False)
    check(g, ids=False)                                                      # the roots' ids go through the work buffer
    check(g, records=False)
    check(g, ids=False, records=False)
    assert check(g, rounds=False)[1] is None
    m = np.diff(g.offsets.astype(np.int64)).astype(np.uint64)
    no_sums = Graph(ctx, g.U, g.lo, g.tg, g.offsets, None)
    check(no_sums)
    assert np.array_equal(no_sums.want()[2][:, 3], no_sums.want()[2][:, 2]) and int(no_sums.want()[2][:, 2].sum()) == int(m.sum())
    no_offsets = Graph(ctx, g.U, g.lo, g.tg, None, g.sums)
    check(no_offsets)
    assert np.array_equal(no_offsets.want()[2][:, 2], no_offsets.want()[2][:, 1])
    neither = Graph(ctx, g.U, g.lo, g.tg, None, None)
    check(neither, ids=False)
    assert np.array_equal(neither.want()[2][:, 3], neither.want()[2][:, 1])


def test_max_components(ctx):
    g = _sparse(ctx, True)
    labels, ids, rec, n = g.want()
    check(g, max_components=n)
    check(g, max_components=n + 7)
    st, got_l, got_i, got_r, got_n, rounds = raw(g, max_components=n - 1)
    assert st == E_NOMEM and got_n == n and rounds >= 1
    assert (got_r == np.uint64(POISON & (2**64 - 1))).all()                  # one short: the records keep their poison
    assert np.array_equal(got_l[:g.U], labels) and np.array_equal(got_i[:g.U], ids) and guards_intact((got_l, g.U), (got_i, g.U))
    st, got_l, got_i, got_r, got_n, _ = raw(g, ids=False, max_components=0)
    assert st == E_NOMEM and got_n == n and np.array_equal(got_l[:g.U], labels)


@pytest.mark.parametrize("which", ("sparse", "chain"))
def test_repeated_calls_give_identical_bytes(ctx, which):
    g = _sparse(ctx, False) if which == "sparse" else _chain(ctx, "permuted")
    a, b = raw(g), raw(g)
    assert a[0] == b[0] == 0 and a[4] == b[4]
    assert all(np.array_equal(x, y) for x, y in zip(a[1:4], b[1:4]))
    assert np.array_equal(a[1][:g.U], g.want()[0])


# ---------------------------------------------------------------- the Python layer on synthetic links
def test_python_layer(ctx):
    import torch

    from kmers_amd.api import UnitigLinks, Unitigs

    g = _sparse(ctx, False)
    labels, ids, rec, n = g.want()
    un = Unitigs(None, g.d["offsets"], None, g.d["sums"], g.U, 31)
    links = UnitigLinks(g.d["lo"], g.d["tg"])
    comp = ctx.count_unitig_components(un, links)
    assert comp.n_components == n and comp.rounds >= 1 and comp.labels.dtype == comp.ids.dtype == torch.int64
    assert np.array_equal(u64(comp.labels), labels) and np.array_equal(u64(comp.ids), ids) and np.array_equal(u64(comp.records), rec)
    assert np.array_equal(u64(comp.roots), rec[:, 0]) and np.array_equal(u64(comp.n_unitigs), rec[:, 1])
    assert np.array_equal(u64(comp.n_nodes), rec[:, 2]) and np.array_equal(u64(comp.count_sums), rec[:, 3])
    s = rec[:, 3].view(np.int64).astype(np.float64)                          # (Unitigs.mean_counts' reading of a u64 word)
    want_mean = np.where(rec[:, 3].view(np.int64) < 0, s + 2.0**64, s) / rec[:, 2].astype(np.float64)
    assert np.array_equal(comp.mean_counts.cpu().numpy(), want_mean)
    for kw in (dict(), dict(min_nodes=60), dict(min_unitigs=3), dict(min_count_sum=2**63), dict(largest=5), dict(largest=40, min_unitigs=4)):
        keep = comp.keep(**kw)
        assert keep.dtype == torch.uint8 and np.array_equal(keep.cpu().numpy(), component_np.keep_np(ids, rec, **kw)), kw
    assert 0 < int(comp.keep(min_unitigs=3).sum()) < g.U
    mask = torch.from_numpy((np.arange(g.U) % 3 != 0)).to(ctx.device)        # a bool mask
    masked = ctx.count_unitig_components(un, links, mask=mask, stats=False)
    want = components_np(g.offsets, g.sums, g.lo, g.tg, (np.arange(g.U) % 3 != 0).astype(np.uint8))
    assert masked.records is None and masked.n_components == want[3]
    assert np.array_equal(u64(masked.labels), want[0]) and np.array_equal(u64(masked.ids), want[1])
    with pytest.raises(ValueError):
        ctx.count_unitig_components(un, links, mask=mask[:-1])
    with pytest.raises(ValueError):
        ctx.count_unitig_components(un, UnitigLinks(g.d["lo"][:-2], g.d["tg"]))


# ---------------------------------------------------------------- real graphs
def _check_linked(x, mask=None):
    links = x.links()
    g = Graph(x.ctx, x.U, u64(links.offsets), u64(links.targets), x.uoff, u64(x.unitigs.count_sums), mask)
    check(g)
    comp = x.ctx.count_unitig_components(x.unitigs, links, mask=None if mask is None else dev(x.ctx, mask))
    labels, ids, rec, n = g.want()
    assert comp.n_components == n and np.array_equal(u64(comp.labels), labels) and np.array_equal(u64(comp.ids), ids)
    assert np.array_equal(u64(comp.records).reshape(-1, 4), rec)
    return g, links


@pytest.mark.parametrize("name", ("backbone", "swapped", "fork", "fork topological", "fork tie"))
@pytest.mark.parametrize("k", (15, 31, 33, 47))
def test_string_cases(ctx, k, name):
    """every string case of the cleaning tests hangs together: one component that holds every unitig and every entry"""
    seqs = cases(k)[name][0]
    d_k, d_c = _count(ctx, k, seqs)
    x = Linked(ctx, k, d_k, d_c)
    g, _ = _check_linked(x)
    assert g.want()[2].tolist() == [[0, x.U, x.n, int(u64(d_c).sum(dtype=np.uint64))]] and x.U > 1


@pytest.mark.parametrize("k", (4, 5, 6, 8))
def test_dense_graph(ctx, k):
    """degrees up to four, self-links, hairpins and (even k) palindromic one-node unitigs whose links go one way only"""
    t = _table(ctx, _dense_reads if k < 8 else _dense8_reads, k)
    deg_max = 0
    for min_count in (1, 2):
        x = Linked(ctx, k, t.d_k, t.d_c, min_count)
        g, links = _check_linked(x)
        deg_max = max(deg_max, int(links.degrees.max()))
        _check_linked(x, (np.arange(x.U) % 4 != 1).astype(np.uint8))
    assert deg_max == 4


@pytest.mark.parametrize("k", (31, 47))
def test_drop_small_components(ctx, k):
    """a backbone and, from a second sequence, a fork of three unitigs: count_simplify keeps the fork -- no rule of the cleaning call
    has anything to say about it -- and the component filter removes it, key for key as the host's references do"""
    seqs, main, _ = fork_cases(k)
    d_k, d_c = _count(ctx, k, seqs)
    tk, tc = table(seqs, k)
    assert np.array_equal(u64(d_k).reshape(tk.shape), tk) and np.array_equal(u64(d_c), tc)
    one = k <= 31
    x = Linked(ctx, k, d_k, d_c)
    g, links = _check_linked(x)
    assert sorted(g.want()[2][:, 1].tolist()) == [1, 3]                      # one component of more than one unitig ...
    for kw in ({}, dict(island_max_nodes=k), dict(tip_ratio=None, island_max_nodes=k)):
        keep, reason = ctx.count_unitig_clean(x.unitigs, links, **kw)
        assert int(reason.sum()) == 0 and int(keep.sum()) == x.U             # ... that every KMX_CLEAN_* rule keeps
    sk, sc, log = (ctx.count_simplify if one else ctx.count_simplify2)(d_k, d_c, k, island_max_nodes=k)
    assert np.array_equal(u64(sk).reshape(tk.shape), tk) and log[0]["removed"] == 0
    drop = ctx.count_drop_small_components if one else ctx.count_drop_small_components2
    min_nodes = len(main) - k + 1
    gk, gc, comp = drop(d_k, d_c, k, min_nodes)
    wk, wc, (labels, ids, rec, n) = component_np.drop_small_np(tk, tc, k, min_nodes)
    assert key_list(u64(gk).reshape(wk.shape)) == key_list(wk) and np.array_equal(u64(gc), wc)
    assert key_list(wk) == key_list(table([(main, 6)], k)[0])               # what is left is the backbone's table
    assert comp.n_components == n == 2 and np.array_equal(u64(comp.ids), ids) and np.array_equal(u64(comp.records), rec)
    gk, gc, _ = drop(d_k, d_c, k, 1)
    assert np.array_equal(u64(gk).reshape(tk.shape), tk) and np.array_equal(u64(gc), tc)


@pytest.mark.parametrize("k", (31, 47))
def test_read_paths_components(ctx, k):
    """reads cut from the two sequences land in two different ids; a read that maps nowhere has no segment"""
    seqs, main, (stem, a, b) = fork_cases(k)
    d_k, d_c = _count(ctx, k, seqs)
    x = Linked(ctx, k, d_k, d_c)
    comp = ctx.count_unitig_components(x.unitigs, x.links())
    L = k + 20
    cut = lambda s, at: np.frombuffer(s[at:at + L].encode(), np.uint8)
    rng = np.random.default_rng(5700 + k)
    reads = [cut(main, 0), cut(main, 200), cut(stem + a, 5), cut(stem + a, 2 * k), cut(stem[-(k - 1):] + b, 10), random_reads(rng, L), cut(main, 400)]
    origin = [0, 0, 1, 1, 1, None, 0]
    bases = ctx.to_device(np.concatenate(reads))
    paths = (ctx.count_read_paths if k <= 31 else ctx.count_read_paths2)(bases, len(reads), L, k, d_k, x.unitigs, place=x.d_place)
    got = paths.components(comp)
    assert got.numel() == paths.n_segments and np.array_equal(got.cpu().numpy(), u64(comp.ids).astype(np.int64)[paths.unitig.cpu().numpy()])
    per_read = {}
    for r, c in zip(paths.read.cpu().tolist(), got.cpu().tolist()):
        per_read.setdefault(r, set()).add(c)
    assert 5 not in per_read and sorted(per_read) == [0, 1, 2, 3, 4, 6]      # the random read has no segment
    ids_of = {o: set().union(*(per_read[r] for r, o2 in enumerate(origin) if o2 == o)) for o in (0, 1)}
    assert len(ids_of[0]) == 1 and len(ids_of[1]) == 1 and ids_of[0] != ids_of[1]


# ---------------------------------------------------------------- the call's conventions
def test_argument_errors(ctx):
    g = _sparse(ctx, False)
    assert raw(g, handle=None)[0] == E_ARG                                   # NULL ctx
    assert raw(g, h_n=False)[0] == E_ARG                                     # NULL h_n_components
    assert raw(g, n_unitigs=2**40 + 1)[0] == E_ARG and raw(g, n_links=2**43 + 1)[0] == E_ARG
    assert raw(g, labels=None)[0] == E_ARG and raw(g, lo=None)[0] == E_ARG   # d_labels, d_link_offsets
    st, got_l, got_i, got_r, _, _ = raw(g, tg=None)                          # d_links NULL with n_links > 0
    assert st == E_ARG
    poison = np.uint64(POISON & (2**64 - 1))
    assert (got_l == poison).all() and (got_i == poison).all() and (got_r == poison).all()   # nothing ran
    # n_unitigs == 0: a no-op that sets the count and the rounds
    st, got_l, got_i, got_r, n, rounds = raw(g, n_unitigs=0)
    assert (st, n, rounds) == (0, 0, 0) and (got_l == poison).all() and (got_i == poison).all() and (got_r == poison).all()
    # no links at all: d_links may be NULL
    alone = Graph(ctx, 10, np.zeros(21, np.uint64), np.zeros(0, np.uint64))
    assert alone.d["tg"] is None and check(alone) == (10, 1)


def test_work_buffer_cap(ctx):
    """the documented working set (kmx.h) is what the call asks for: one byte less is KMX_E_NOMEM before anything is written"""
    g = _sparse(ctx, False)
    a256 = lambda v: (v + 255) // 256 * 256
    base = a256(8 * ((g.U + 4095) // 4096 + 1)) + 256
    poison = np.uint64(POISON & (2**64 - 1))
    try:
        for kw, need in ((dict(), base), (dict(ids=False), base + a256(8 * g.U)), (dict(ids=False, records=False), base)):
            ctx.set_work_buffer_limit(need - 1)
            allocs0 = ctx.work_buffer_info()[1]
            st, got_l, got_i, got_r, _, _ = raw(g, **kw)
            assert st == E_NOMEM and ctx.work_buffer_info()[1] == allocs0, kw
            assert all(x is None or (x == poison).all() for x in (got_l, got_i, got_r)), kw
            ctx.set_work_buffer_limit(need)                                  # exactly the documented size: served
            check(g, **kw)
    finally:
        ctx.set_work_buffer_limit(0)


@pytest.mark.parametrize("k", (15, 33))
def test_empty_table(ctx, k):
    import torch

    kmers = torch.zeros((0,) if k <= 31 else (0, 2), dtype=torch.int64, device=ctx.device)
    counts = torch.zeros(0, dtype=torch.int64, device=ctx.device)
    x = Linked(ctx, k, kmers, counts)
    comp = ctx.count_unitig_components(x.unitigs, x.links())
    assert comp.n_components == 0 and comp.rounds == 0 and comp.labels.numel() == 0 and comp.records.shape == (0, 4)
    assert comp.keep(min_nodes=5).numel() == 0 and comp.mean_counts.numel() == 0
