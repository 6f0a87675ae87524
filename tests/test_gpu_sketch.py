"""The counting sketch on the GPU (kmx_sketch_*, kmx_count_canonical_min(2), Context.count_solid; kmx_sketch.hip).

Every comparison is byte-exact against the host model tests/sketch_np.py (pinned on the CPU by tests/test_sketch_np.py): the
sketch a call leaves, the estimates, the merged sketch, the statistics, the filtered tables.  The keys the model is fed are the
canon / flags of kmx_canonical_windows(2), which the oracle pins elsewhere; expected tables come from count_np.table_of.  Shapes
are the smallest at which the kernels can go wrong: one block (every cell contended, the shift by 64), saturation, ragged and
misaligned and long reads, more keys than one grid sweep, a second stream."""
import ctypes as C

import numpy as np
import pytest

from kmers_amd import _lib
from tests import sketch_np as sk
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import random_reads, table_of, u64

pytestmark = pytest.mark.gpu


def _cells(s):
    return s.cells.cpu().numpy()


def _keys(rng, n, words):
    a = rng.integers(0, 2**64, (n, words), dtype=np.uint64)
    return a[:, 0] if words == 1 else a


def _dev(ctx, a):
    return ctx.to_device(np.ascontiguousarray(a))


def _add_words(ctx, s, keys, weights=None):
    f = ctx.sketch_add_words if keys.ndim == 1 else ctx.sketch_add_words2
    return f(s, _dev(ctx, keys), None if weights is None else _dev(ctx, np.asarray(weights, np.uint64)))


def _windows(ctx, bases, n, L, k, offsets=None, host_offsets=None):
    """canon ((windows,) or (windows, 2) uint64) and flags of the batch on the host, from the device's windows call"""
    if k <= 31:
        o = ctx.canonical_windows(bases, n, L, k, offsets=offsets, host_offsets=host_offsets, want=("canon", "flags"))
        return u64(o["canon"]), o["flags"].cpu().numpy()
    o = ctx.canonical_windows2(bases, n, L, k, offsets=offsets, host_offsets=host_offsets)
    return u64(o["canon"]).reshape(-1, 2), o["flags"].cpu().numpy()


# ---------------------------------------------------------------- add_words: contention, saturation, weights
@pytest.mark.parametrize("words", (1, 2))
@pytest.mark.parametrize("log2_blocks", (0, 1, 10))
def test_add_words_matches_the_model(ctx, words, log2_blocks):
    rng = np.random.default_rng(10 * log2_blocks + words)
    keys = _keys(rng, 5000, words)
    keys[1::7] = keys[0]                                    # one heavy key among them
    s = _add_words(ctx, ctx.sketch_new(log2_blocks, seed=11), keys)
    exp = sk.add(sk.new(log2_blocks), keys, log2_blocks, seed=11)
    assert (_cells(s) == exp).all()
    if log2_blocks == 0:
        assert exp.min() > 0 and (exp == 255).sum() >= 4    # every cell contended, some saturated
    w = rng.integers(0, 300, len(keys)).astype(np.uint64)   # weights: 0 adds nothing, above 255 is 255
    s = _add_words(ctx, s, keys, w)
    exp = sk.add(exp, keys, log2_blocks, seed=11, weights=w)
    assert (_cells(s) == exp).all()
    f = ctx.sketch_lookup if words == 1 else ctx.sketch_lookup2
    assert (f(s, _dev(ctx, keys)).cpu().numpy() == sk.estimate(exp, keys, log2_blocks, seed=11)).all()


def test_saturation(ctx):
    n_win, k = 300, 31
    s = ctx.sketch_add(ctx.sketch_new(4), _dev(ctx, np.full(n_win + k - 1, ord("A"), np.uint8)), 1, n_win + k - 1, k)
    got, cells = _cells(s), sk.cells_of(np.zeros(1, np.uint64), 4)[0]
    assert (got[cells] == 255).all() and np.count_nonzero(got) == 4          # AAA...A is canonical word 0
    key = np.array([0x0123456789ABCDEF], np.uint64)
    s = ctx.sketch_new(4, seed=3)
    _add_words(ctx, s, key, [200])
    assert np.count_nonzero(_cells(s) == 200) == 4
    _add_words(ctx, s, key, [200])
    got, cells = _cells(s), sk.cells_of(key, 4, seed=3)[0]
    assert (got[cells] == 255).all() and np.count_nonzero(got) == 4
    s = _add_words(ctx, ctx.sketch_new(4, seed=3), key, [2**40 + 1])         # a u64 weight above 255
    assert (_cells(s) == got).all()


# ---------------------------------------------------------------- sketch_add == add_words over the windows call
def _read_cases(rng, k):
    n, L = 300, 150
    yield "uniform", random_reads(rng, n * L), n, L, None, 0
    lens = rng.integers(0, 161, 400)
    lens[::17] = 0
    lens[5::13] = k - 1
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    yield "ragged", random_reads(rng, int(offsets[-1])), 400, 160, offsets, 0
    h = random_reads(rng, n * L)
    h[rng.random(n * L) < 0.004] = ord("N")
    low = rng.random(n * L) < 0.3
    h[low & (h != ord("N"))] |= 0x20
    yield "dirty", h, n, L, None, 0
    yield "misaligned", random_reads(rng, n * L), n, L, None, 3
    yield "long", random_reads(rng, 1000), 1, 1000, None, 0


@pytest.mark.parametrize("k", (21, 31, 33, 64))
def test_sketch_add_equals_add_words_over_the_windows(ctx, k):
    rng = np.random.default_rng(500 + k)
    add = ctx.sketch_add if k <= 31 else ctx.sketch_add2
    lookup_reads = ctx.sketch_lookup_reads if k <= 31 else ctx.sketch_lookup_reads2
    lb = 8
    for name, host, n, L, offsets, shift in _read_cases(rng, k):
        buf = _dev(ctx, np.concatenate([np.zeros(shift, np.uint8), host, np.zeros(16, np.uint8)]))
        bases = buf[shift:shift + len(host)]
        d_off = None if offsets is None else _dev(ctx, offsets)
        canon, flags = _windows(ctx, bases, n, L, k, offsets=d_off, host_offsets=offsets)
        assert (flags & 1).any(), name
        exp = sk.add(sk.new(lb), canon, lb, seed=k, flags=flags)
        s = add(ctx.sketch_new(lb, seed=k), bases, n, L, k, offsets=d_off)
        assert (_cells(s) == exp).all(), (name, k)
        via_words = ctx.sketch_new(lb, seed=k)
        _add_words(ctx, via_words, canon[(flags & 1) != 0])
        assert (_cells(via_words) == exp).all(), (name, k)
        # lookup_reads: one byte per slot, invalid slots 0
        est = lookup_reads(s, bases, n, L, k, offsets=d_off).cpu().numpy()
        assert (est == sk.estimate(exp, canon, lb, seed=k, flags=flags)).all(), (name, k)
        if name == "dirty":
            assert ((flags & 1) == 0).any() and (est[(flags & 1) == 0] == 0).all()
    s = ctx.sketch_new(lb)
    add(s, None, 0, 150, k)                                   # n_reads = 0 leaves the sketch untouched
    add(s, _dev(ctx, random_reads(rng, 40 * (k - 1))), 40, k - 1, k)   # so do reads without a window
    assert not _cells(s).any()


# ---------------------------------------------------------------- more keys than one grid sweep; streams
def test_past_one_sweep_repeats_and_other_stream(ctx):
    import torch

    from kmers_amd.api import Context

    n_cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    sweep = n_cu * _lib.SKETCH_SWEEP_LANES_PER_CU
    n = sweep + sweep // 8 + 77                               # about 3e5 on 256 compute units
    rng = np.random.default_rng(9)
    keys = _keys(rng, n, 1)
    keys[sweep:] = keys[:n - sweep]                           # the second sweep's keys hit cells of the first's
    keys2 = np.stack([keys, keys[::-1]], axis=1)
    lb = 8                                                    # 16 384 cells for 1.2e6 adds: contended throughout, few saturated
    exp, exp2 = sk.add(sk.new(lb), keys, lb, seed=1), sk.add(sk.new(lb), keys2, lb, seed=1)
    a = _add_words(ctx, ctx.sketch_new(lb, seed=1), keys)
    b = _add_words(ctx, ctx.sketch_new(lb, seed=1), keys)
    assert (_cells(a) == exp).all() and (_cells(b) == exp).all()
    assert (_cells(_add_words(ctx, ctx.sketch_new(lb, seed=1), keys2)) == exp2).all()
    assert (ctx.sketch_lookup(a, _dev(ctx, keys)).cpu().numpy() == sk.estimate(exp, keys, lb, seed=1)).all()
    other = Context(stream=torch.cuda.Stream())
    try:
        c = _add_words(other, other.sketch_new(lb, seed=1), keys)
        other.synchronize()
        assert (_cells(c) == exp).all()
    finally:
        other.close()
    # a roomier sketch over the same keys: few collisions, every weight counted once
    lb = 12
    assert (_cells(_add_words(ctx, ctx.sketch_new(lb), keys)) == sk.add(sk.new(lb), keys, lb)).all()


# ---------------------------------------------------------------- merge and stats
def test_merge_law_and_aliasing(ctx):
    rng = np.random.default_rng(21)
    n, L, k, lb = 600, 150, 31, 5
    host = random_reads(rng, n * L)
    host.reshape(n, L)[::3] = host[:L]                        # a repeated read: cells that saturate in the whole, not in a half
    half = (n // 2) * L
    whole = ctx.sketch_add(ctx.sketch_new(lb, seed=2), _dev(ctx, host), n, L, k)
    a = ctx.sketch_add(ctx.sketch_new(lb, seed=2), _dev(ctx, host[:half]), n // 2, L, k)
    b = ctx.sketch_add(ctx.sketch_new(lb, seed=2), _dev(ctx, host[half:]), n - n // 2, L, k)
    ea, eb = _cells(a), _cells(b)
    assert _cells(whole).max() == 255 and (sk.merge(ea, eb) == _cells(whole)).all()
    assert (_cells(ctx.sketch_merge(a, b)) == _cells(whole)).all()
    assert (_cells(a) == ea).all() and (_cells(b) == eb).all()
    assert ctx.sketch_merge(a, b, out=a) is a and (_cells(a) == _cells(whole)).all()     # d_out aliasing d_a
    a2 = ctx.sketch_add(ctx.sketch_new(lb, seed=2), _dev(ctx, host[:half]), n // 2, L, k)
    ctx.sketch_merge(a2, b, out=b)                                                        # d_out aliasing d_b
    assert (_cells(b) == _cells(whole)).all()
    with pytest.raises(ValueError):
        ctx.sketch_merge(a, ctx.sketch_new(lb, seed=3))


@pytest.mark.parametrize("log2_blocks", (0, 7, 13))
def test_stats_accumulate(ctx, log2_blocks):
    rng = np.random.default_rng(31 + log2_blocks)
    keys = _keys(rng, 40000, 1)
    keys[::5] = keys[0]
    s = _add_words(ctx, ctx.sketch_new(log2_blocks), keys)
    exp = np.bincount(_cells(s), minlength=256).astype(np.uint64)
    hist = ctx.sketch_stats(s)
    assert (u64(hist) == exp).all() and int(exp.sum()) == 64 << log2_blocks
    assert (u64(ctx.sketch_stats(s, out=hist)) == 2 * exp).all()
    assert s.fill() == 1.0 - int(exp[0]) / (64 << log2_blocks)


# ---------------------------------------------------------------- count_canonical_min
@pytest.mark.parametrize("k", (31, 47))
def test_count_canonical_min(ctx, k):
    rng = np.random.default_rng(700 + k)
    n, L, lb, seed = 500, 150, 14, 5
    host = random_reads(rng, n * L)
    host.reshape(n, L)[::2] = host.reshape(n, L)[1::2]                # every read twice: counts of 2
    host.reshape(n, L)[:40] = host.reshape(n, L)[41]                  # one read forty times: counts well above 3
    host.reshape(n, L)[::6, 75] = ord("N")                            # windows that are skipped: their twins' k-mers occur once
    bases = _dev(ctx, host)
    two = k > 31
    add, cmin, full = ((ctx.sketch_add2, ctx.count_canonical_min2, ctx.count_canonical2) if two else
                       (ctx.sketch_add, ctx.count_canonical_min, ctx.count_canonical))
    canon, flags = _windows(ctx, bases, n, L, k)
    s = add(ctx.sketch_new(lb, seed=seed), bases, n, L, k)
    es = _cells(s)
    fk, fc = full(bases, n, L, k)
    shape = (-1, 2) if two else (-1,)
    for min_est in (0, 1):                                            # a sketch that has seen the batch: the unfiltered table
        gk, gc = cmin(s, min_est, bases, n, L, k)
        assert (u64(gk) == u64(fk)).all() and (u64(gc) == u64(fc)).all() and gk.shape == fk.shape
    for min_est in (256, 2**32 - 1):
        gk, gc = cmin(s, min_est, bases, n, L, k)
        assert gk.shape[0] == 0 and gc.numel() == 0
        assert cmin(s, min_est, bases, n, L, k, count_only=True) == 0
    sizes = {}
    for min_est in (2, 3):
        ek, ec = sk.table_min(es, canon, flags, lb, seed, min_est)
        gk, gc = cmin(s, min_est, bases, n, L, k)
        assert u64(gk).reshape(shape).shape == ek.shape
        assert (u64(gk).reshape(shape) == ek).all() and (u64(gc) == ec).all()
        assert cmin(s, min_est, bases, n, L, k, count_only=True) == len(ec)
        sizes[min_est] = len(ec)
    assert 0 < sizes[3] < sizes[2] < fc.numel()
    # one entry too few: KMX_E_NOMEM, the count reported, nothing written
    nd = sizes[2]
    km = _dev(ctx, np.full((2 if two else 1) * nd, 0x5A5A5A5A5A5A5A5A, np.uint64))
    cn = _dev(ctx, np.full(nd, 0x5A5A5A5A5A5A5A5A, np.uint64))
    got = C.c_uint64(0)
    r = ctx._reads(bases, n, L, None)
    fn = ctx.lib.kmx_count_canonical_min2 if two else ctx.lib.kmx_count_canonical_min
    st = fn(ctx._h, C.byref(r), k, C.c_void_p(s.cells.data_ptr()), lb, seed, 2, C.c_void_p(km.data_ptr()), C.c_void_p(cn.data_ptr()), nd - 1,
            C.byref(got))
    ctx.synchronize()
    assert st == _lib.E_NOMEM and got.value == nd
    assert (u64(km) == 0x5A5A5A5A5A5A5A5A).all() and (u64(cn) == 0x5A5A5A5A5A5A5A5A).all()
    # the plain counter is what it was
    gk, gc = full(bases, n, L, k)
    ek, ec = table_of(canon, flags)
    assert (u64(gk).reshape(shape) == ek).all() and (u64(gc) == ec).all()


# ---------------------------------------------------------------- end to end: count_solid
@pytest.fixture(scope="module")
def solid_reads():
    return sk.solid_batches(2024)


@pytest.mark.parametrize("k", (31, 47))
def test_count_solid_end_to_end(ctx, solid_reads, k):
    two = k > 31
    solid, full, flt = ((ctx.count_solid2, ctx.count_canonical2, ctx.count_filter2) if two else
                        (ctx.count_solid, ctx.count_canonical, ctx.count_filter))
    batches = [(_dev(ctx, b), len(o) - 1, 160, _dev(ctx, o)) for b, o in solid_reads]
    all_bases = np.concatenate([b for b, _ in solid_reads])
    all_offsets = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(o.astype(np.int64)) for _, o in solid_reads]))]).astype(np.uint64)
    ek, ec = flt(*full(_dev(ctx, all_bases), len(all_offsets) - 1, 160, k, offsets=_dev(ctx, all_offsets)), 2, 2**64 - 1)
    assert ec.numel() > 10000
    # deliberately undersized: false positives occur and are harmless
    sizes12 = []
    gk, gc, s = solid(batches, k, 2, log2_blocks=12, tables=sizes12)
    assert gk.shape == ek.shape and (u64(gk) == u64(ek)).all() and (u64(gc) == u64(ec)).all()
    assert s.fill() > 0.9
    unfiltered = [int(full(*b[:3], k, offsets=b[3])[1].numel()) for b in batches]
    # sized for the data: the same table, and batch tables that never held the singletons
    sizes18 = []
    gk, gc, s = solid(batches, k, 2, log2_blocks=18, tables=sizes18)
    assert gk.shape == ek.shape and (u64(gk) == u64(ek)).all() and (u64(gc) == u64(ec)).all()
    assert max(sizes18) < max(unfiltered) and all(a <= b for a, b in zip(sizes18, unfiltered))
    assert max(sizes18) < max(sizes12) <= max(unfiltered)             # the false positives of the small sketch were there
    # and it is the host model's sketch
    canon = [_windows(ctx, b[0], b[1], 160, k, offsets=b[3], host_offsets=o) for b, (_, o) in zip(batches, solid_reads)]
    _, _, es, esizes = sk.count_solid(canon, 2, 18)
    assert (_cells(s) == es).all() and esizes == sizes18
    with pytest.raises(ValueError):
        solid(batches, k, 0, log2_blocks=12)
    with pytest.raises(ValueError):
        solid(batches, k, 256, log2_blocks=12)


# ---------------------------------------------------------------- argument errors
def test_argument_errors(ctx):
    rng = np.random.default_rng(1)
    lib, h = ctx.lib, ctx._h
    s = ctx.sketch_new(3)
    keys = _dev(ctx, _keys(rng, 64, 1))
    est = ctx.sketch_lookup(s, keys)
    bases = _dev(ctx, random_reads(rng, 10 * 150))
    r = ctx._reads(bases, 10, 150, None)
    p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)   # noqa: E731
    nd = C.c_uint64(0)
    before = _cells(s).copy()
    # a misaligned d_sketch
    assert lib.kmx_sketch_add_words(h, p(keys), None, 64, p(s.cells, 16), 2, 0) == _lib.E_ARG
    assert lib.kmx_sketch_add(h, C.byref(r), 31, p(s.cells, 1), 2, 0) == _lib.E_ARG
    assert lib.kmx_sketch_lookup(h, p(keys), 64, p(s.cells, 32), 2, 0, p(est)) == _lib.E_ARG
    assert lib.kmx_sketch_stats(h, p(s.cells, 8), 2, p(keys)) == _lib.E_ARG
    assert lib.kmx_sketch_merge(h, p(s.cells), p(s.cells, 4), 2, p(s.cells)) == _lib.E_ARG
    assert lib.kmx_count_canonical_min(h, C.byref(r), 31, p(s.cells, 2), 2, 0, 2, None, None, 0, C.byref(nd)) == _lib.E_ARG
    # log2_blocks = 33
    assert lib.kmx_sketch_add_words(h, p(keys), None, 64, p(s.cells), 33, 0) == _lib.E_ARG
    assert lib.kmx_sketch_add2(h, C.byref(r), 47, p(s.cells), 33, 0) == _lib.E_ARG
    assert lib.kmx_sketch_lookup_reads(h, C.byref(r), None, 31, p(s.cells), 33, 0, p(est)) == _lib.E_ARG
    assert lib.kmx_sketch_merge(h, p(s.cells), p(s.cells), 33, p(s.cells)) == _lib.E_ARG
    assert lib.kmx_count_canonical_min2(h, C.byref(r), 47, p(s.cells), 33, 0, 2, None, None, 0, C.byref(nd)) == _lib.E_ARG
    # k = 32, and each width's calls outside their range
    for fn in (lib.kmx_sketch_add, lib.kmx_sketch_add2):
        assert fn(h, C.byref(r), 32, p(s.cells), 3, 0) == _lib.E_K_RANGE
    assert lib.kmx_sketch_add(h, C.byref(r), 33, p(s.cells), 3, 0) == _lib.E_K_RANGE
    assert lib.kmx_sketch_add2(h, C.byref(r), 31, p(s.cells), 3, 0) == _lib.E_K_RANGE
    assert lib.kmx_sketch_lookup_reads(h, C.byref(r), None, 32, p(s.cells), 3, 0, p(est)) == _lib.E_K_RANGE
    assert lib.kmx_sketch_lookup_reads2(h, C.byref(r), None, 32, p(s.cells), 3, 0, p(est)) == _lib.E_K_RANGE
    assert lib.kmx_count_canonical_min(h, C.byref(r), 32, p(s.cells), 3, 0, 2, None, None, 0, C.byref(nd)) == _lib.E_K_RANGE
    assert lib.kmx_count_canonical_min2(h, C.byref(r), 32, p(s.cells), 3, 0, 2, None, None, 0, C.byref(nd)) == _lib.E_K_RANGE
    # a NULL sketch with work to do; without work it is a no-op
    assert lib.kmx_sketch_add_words(h, p(keys), None, 64, None, 3, 0) == _lib.E_ARG
    assert lib.kmx_sketch_add(h, C.byref(r), 31, None, 3, 0) == _lib.E_ARG
    assert lib.kmx_sketch_lookup(h, p(keys), 64, None, 3, 0, p(est)) == _lib.E_ARG
    assert lib.kmx_count_canonical_min(h, C.byref(r), 31, None, 3, 0, 2, None, None, 0, C.byref(nd)) == _lib.E_ARG
    assert lib.kmx_sketch_add_words(h, None, None, 0, None, 3, 0) == _lib.OK
    # a misaligned two-word key array
    assert lib.kmx_sketch_add_words2(h, p(keys, 8), None, 8, p(s.cells), 3, 0) == _lib.E_ARG
    ctx.synchronize()
    assert (_cells(s) == before).all()
