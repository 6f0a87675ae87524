"""Per-read abundance statistics against a count table on the GPU: kmx_count_read_stats(2) (kmx_count_read_stats.hip).

Every comparison is u64 equality of whole (n_reads, 8) arrays.  Expected values are made on the host: the oracle's canonical words
and flags of the batch, a host lookup (lower bound + equality: tests/count_np.py), and a plain per-read loop over the eight fields
as kmx.h defines them, written here.  Tables are np.unique of the oracle's valid words of a batch A with every third entry dropped -- except the
k-mers of a few reads that both batches hold, so that some reads are wholly in the table; batch B shares every second read with A.
Every table-driven test asserts of its own input: at least a tenth of the valid windows hit and a tenth miss, one read has a span
shorter than its window count, one has a span over all its windows, n_valid is even in one read and odd in another.
At a size the oracle does not reach the expectation is the pinned composition count_lookup_reads(2) + canonical_windows(2) flags,
reduced over the reshaped (n, W) array by a second, vectorised host implementation."""
import ctypes as C

import numpy as np
import pytest

from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import host_lookup, orc_windows, random_reads, table_of, u64

pytestmark = pytest.mark.gpu

U64_MAX = 2**64 - 1
POISON = -0x5A5A5A5A5A5A5A5B


def _host_stats(cnt, flags, wo, solid_min):
    """the eight fields of kmx.h, read by read"""
    n = len(wo) - 1
    out = np.zeros((n, 8), np.uint64)
    sm = np.uint64(solid_min)
    for r in range(n):
        c = cnt[int(wo[r]):int(wo[r + 1])]
        v = (flags[int(wo[r]):int(wo[r + 1])] & 1) != 0
        cv = c[v]
        nv = len(cv)
        out[r, 0] = nv
        if nv:
            out[r, 1] = int((cv != 0).sum())
            out[r, 2] = int((cv >= sm).sum())
            out[r, 3] = cv.min()
            out[r, 4] = cv.max()
            out[r, 5] = sum(int(x) for x in cv.tolist()) & U64_MAX
            out[r, 6] = np.sort(cv)[nv // 2]
        best_len, best_start, run = 0, 0, 0
        for p, s in enumerate((v & (c >= sm)).tolist()):
            run = run + 1 if s else 0
            if run > best_len:                   # (strictly longer: the earliest run wins ties)
                best_len, best_start = run, p - run + 1
        out[r, 7] = (best_len << 32) | best_start
    return out


def _dense_stats(cnt, flags, n, W, solid_min):
    """the same fields of uniform reads, vectorised over the (n, W) arrays: an implementation of its own"""
    c = cnt.reshape(n, W)
    v = (flags.reshape(n, W) & 1) != 0
    sm = np.uint64(solid_min)
    out = np.zeros((n, 8), np.uint64)
    nv = v.sum(1)
    out[:, 0] = nv
    out[:, 1] = (v & (c != 0)).sum(1)
    solid = v & (c >= sm)
    out[:, 2] = solid.sum(1)
    out[:, 3] = np.where(nv > 0, np.where(v, c, np.uint64(U64_MAX)).min(1), 0)
    out[:, 4] = np.where(v, c, np.uint64(0)).max(1)
    out[:, 5] = np.where(v, c, np.uint64(0)).sum(1, dtype=np.uint64)
    srt = np.sort(np.where(v, c, np.uint64(U64_MAX)), axis=1)
    out[:, 6] = np.where(nv > 0, srt[np.arange(n), np.minimum(nv // 2, W - 1)], 0)
    idx = np.arange(W, dtype=np.int64)[None, :]
    run = idx - np.maximum.accumulate(np.where(solid, -1, idx), axis=1)
    key = np.where(run > 0, (run.astype(np.uint64) << np.uint64(32)) | (0xFFFFFFFF - (idx - run + 1)).astype(np.uint64), np.uint64(0)).max(1)
    out[:, 7] = np.where(key > 0, (key & np.uint64(0xFFFFFFFF00000000)) | (np.uint64(0xFFFFFFFF) - (key & np.uint64(0xFFFFFFFF))), 0)
    return out


def _assert_input(expect, cnt, flags, wo):
    """what every table-driven test asks of its own input"""
    valid = (flags & 1) != 0
    nv = int(valid.sum())
    hits = int((cnt[valid] != 0).sum())
    assert nv > 0 and 10 * hits >= nv and 10 * (nv - hits) >= nv, (nv, hits)
    nwin = np.diff(wo.astype(np.int64))
    span_len = (expect[:, 7] >> np.uint64(32)).astype(np.int64)
    assert ((span_len < nwin) & (nwin > 0)).any(), "no read with a span shorter than its windows"
    assert ((span_len == nwin) & (nwin > 0)).any(), "no read with a span over all its windows"
    n_valid = expect[:, 0].astype(np.int64)
    assert (n_valid % 2 == 0).any() and (n_valid % 2 == 1).any(), "n_valid of one parity only"


def _thin(tk, tc, protect):
    """every third entry dropped, except the keys in `protect` (canonical words, one row each): still a table"""
    keep = np.arange(len(tk)) % 3 != 1
    if tk.ndim == 1:
        keep |= np.isin(tk, protect)
    else:
        held = {(int(a), int(b)) for a, b in protect.tolist()}
        keep |= np.fromiter(((int(a), int(b)) in held for a, b in tk.tolist()), bool, len(tk))
    return tk[keep], tc[keep]


def _uniform_batches(rng, n, L):
    """A and B.  Every second read of B is a read of A; read 0 (shared) is A / T only, so that it is whole in a table of one key at
    k = 1; read 1 of B has an N at base 0 (one window fewer than its neighbours: both parities of n_valid)."""
    a = random_reads(rng, n * L)
    b = random_reads(rng, n * L)
    a.reshape(n, L)[0] = rng.choice(np.frombuffer(b"AT", np.uint8), L)
    b.reshape(n, L)[::2] = a.reshape(n, L)[::2]
    b.reshape(n, L)[1, 0] = ord("N")
    return a, b


def _table_for(orc, a, b, n, L, k, offsets=None, protect_reads=(0,)):
    """the thinned table of batch A that keeps the k-mers of B's `protect_reads` (reads both batches hold)"""
    q, qf = orc_windows(orc, b, n, L, k, offsets)
    wo = orc.win_offsets_for(n, L, k, None if offsets is None else np.asarray(offsets, np.uint64))
    rows = np.concatenate([np.arange(int(wo[r]), int(wo[r + 1])) for r in protect_reads]).astype(np.int64)
    rows = rows[(qf[rows] & 1) != 0]
    tk, tc = table_of(*orc_windows(orc, a, n, L, k, offsets))
    return _thin(tk, tc, q[rows]), (q, qf, wo)


def _call(ctx, k, bases, n, L, d_tk, d_tc, solid_min, d_off=None, out=None):
    f = ctx.count_read_stats if k <= 31 else ctx.count_read_stats2
    return f(bases, n, L, k, d_tk, d_tc, solid_min=solid_min, offsets=d_off, out=out)


def _check(ctx, table, windows, host, n, L, k, offsets=None, solid_mins=(1,), shift=0, conditions=True):
    """the device rows against the host loop for every solid_min; returns the expectation of the first"""
    tk, tc = table
    q, qf, wo = windows
    cnt = host_lookup(tk, tc, q, qf)
    d_tk = ctx.to_device(tk)
    d_tc = None if tc is None else ctx.to_device(tc)
    buf = ctx.to_device(np.concatenate([np.zeros(shift, np.uint8), host, np.zeros(16, np.uint8)]))
    bases = buf[shift:shift + len(host)]
    d_off = None if offsets is None else ctx.to_device(np.asarray(offsets, np.uint64))
    first = None
    for sm in solid_mins:
        expect = _host_stats(cnt, qf, wo, sm)
        got = u64(_call(ctx, k, bases, n, L, d_tk, d_tc, sm, d_off))
        assert got.shape == expect.shape
        bad = np.nonzero((got != expect).any(axis=1))[0]
        assert len(bad) == 0, (k, L, n, sm, shift, bad[:5], got[bad[:2]], expect[bad[:2]])
        if first is None:
            first = expect
    if conditions:
        _assert_input(first, cnt, qf, wo)
    return first


# ---------------------------------------------------------------- uniform reads
@pytest.mark.parametrize("k", (1, 5, 13, 31, 33, 35, 47, 64))
def test_uniform_150(ctx, orc, k):
    rng = np.random.default_rng(7100 + k)
    n, L = 257, 150
    a, b = _uniform_batches(rng, n, L)
    table, win = _table_for(orc, a, b, n, L, k)
    _check(ctx, table, win, b, n, L, k, solid_mins=(1, 2, 0))
    _check(ctx, table, win, b, n, L, k, shift=1, conditions=False)          # odd d_bases


@pytest.mark.parametrize("k", (13, 31, 33))
def test_uniform_36(ctx, orc, k):
    rng = np.random.default_rng(7200 + k)
    n, L = 200, 36
    a, b = _uniform_batches(rng, n, L)
    table, win = _table_for(orc, a, b, n, L, k)
    _check(ctx, table, win, b, n, L, k, solid_mins=(1, 2))


@pytest.mark.parametrize("k", (31, 47))
def test_uniform_1000_segment_route(ctx, orc, k):
    rng = np.random.default_rng(7300 + k)
    n, L = 70, 1000
    a, b = _uniform_batches(rng, n, L)
    b.reshape(n, L)[3, 500] = ord("N")
    table, win = _table_for(orc, a, b, n, L, k, protect_reads=(0, 2))
    _check(ctx, table, win, b, n, L, k, solid_mins=(1, 2, 0))
    _check(ctx, table, win, b, n, L, k, shift=1, conditions=False)


@pytest.mark.parametrize("k", (31, 47))
def test_uniform_block_sized_reads(ctx, orc, k):
    """reads of more than 8192 windows: a whole block per read"""
    rng = np.random.default_rng(7400 + k)
    n, L = 4, 9000
    a, b = _uniform_batches(rng, n, L)
    b.reshape(n, L)[3, 4000] = ord("N")
    table, win = _table_for(orc, a, b, n, L, k)
    _check(ctx, table, win, b, n, L, k, solid_mins=(1, 0))


@pytest.mark.parametrize("k", (13, 31, 47))
def test_uniform_one_window_and_none(ctx, orc, k):
    import torch

    rng = np.random.default_rng(7500 + k)
    n = 300
    a, b = _uniform_batches(rng, n, k)
    table, win = _table_for(orc, a, b, n, k, k)
    _check(ctx, table, win, b, n, k, k, solid_mins=(1, 2))                     # read_len == k: one window
    # read_len == k - 1: no window, every row zero -- and written
    L = k - 1
    out = torch.full((8 * n,), POISON, dtype=torch.int64, device=ctx.device)
    got = _call(ctx, k, ctx.to_device(b[:n * L]), n, L, ctx.to_device(table[0]), ctx.to_device(table[1]), 1, out=out)
    assert got.data_ptr() == out.data_ptr() and got.shape == (n, 8)
    assert (out == 0).all()


# ---------------------------------------------------------------- dirty reads
@pytest.mark.parametrize("k", (13, 31, 47))
def test_dirty_reads(ctx, orc, k):
    rng = np.random.default_rng(7600 + k)
    n, L = 300, 150
    a, b = _uniform_batches(rng, n, L)
    rows = b.reshape(n, L)
    for r in np.nonzero(rng.random(n) < 0.1)[0]:
        if r >= 10:
            rows[r, int(rng.integers(0, L))] = ord("N") if r % 3 else ord(">")
    rows[3, 0] = ord(">")                      # at base 0
    rows[5, L - 1] = ord("N")                  # at the last base
    rows[7, :] = ord("N")                      # all N
    rows[9, :L - k] = ord("N")                 # valid only in its last k bases
    low = rng.random(n * L) < 0.3              # lower case is valid
    b[low & (b != ord("N")) & (b != ord(">"))] |= 0x20
    table, win = _table_for(orc, a, b, n, L, k)
    e = _check(ctx, table, win, b, n, L, k, solid_mins=(1, 2, 0))
    assert (e[7] == 0).all() and int(e[9, 0]) == 1 and int(e[3, 0]) == L - k and int(e[5, 0]) == L - k


# ---------------------------------------------------------------- ragged reads, no window offsets from the caller
def _ragged_mix(rng, k, hi=None):
    special = [0, k - 1, k, k + 1, k + 62, k + 63, k + 64, k + 254, k + 255, k + 256, 1000, 5000]
    if hi is not None:
        special = [x for x in special if x <= hi]
    lens = np.concatenate([special, rng.integers(50, (hi or 200) + 1, 300)]).astype(np.int64)
    rng.shuffle(lens)
    return lens


def _ragged_batches(rng, lens, k):
    """A and B over the same offsets: the first half of the reads shared, and the three longest; 0.2 % of B's bytes N, the longest
    read but two kept clean"""
    n = len(lens)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    a = random_reads(rng, int(offsets[-1]))
    b = random_reads(rng, int(offsets[-1]))
    half = int(offsets[n // 2])
    b[:half] = a[:half]
    order = np.argsort(lens, kind="stable")
    protect = [int(order[-1]), int(order[-2]), int(order[-3])]
    for r in protect:
        b[int(offsets[r]):int(offsets[r + 1])] = a[int(offsets[r]):int(offsets[r + 1])]
    b[rng.random(len(b)) < 0.002] = ord("N")
    r = protect[2]
    b[int(offsets[r]):int(offsets[r + 1])] = a[int(offsets[r]):int(offsets[r + 1])]
    return a, b, offsets, protect


@pytest.mark.parametrize("k", (13, 31, 47))
@pytest.mark.parametrize("bound", (0, 5000))
def test_ragged_mix(ctx, orc, k, bound):
    rng = np.random.default_rng(7700 + k)
    lens = _ragged_mix(rng, k)
    n = len(lens)
    a, b, offsets, protect = _ragged_batches(rng, lens, k)
    table, win = _table_for(orc, a, b, n, bound, k, offsets, protect_reads=protect)
    _check(ctx, table, win, b, n, bound, k, offsets, solid_mins=(1, 2, 0))
    _check(ctx, table, win, b, n, bound, k, offsets, shift=1, conditions=False)     # the misaligned route


@pytest.mark.parametrize("k", (13, 31, 47))
def test_ragged_bound_150(ctx, orc, k):
    rng = np.random.default_rng(7800 + k)
    lens = _ragged_mix(rng, k, hi=150)
    n = len(lens)
    a, b, offsets, protect = _ragged_batches(rng, lens, k)
    table, win = _table_for(orc, a, b, n, 150, k, offsets, protect_reads=protect)
    _check(ctx, table, win, b, n, 150, k, offsets, solid_mins=(1, 2, 0))
    _check(ctx, table, win, b, n, 150, k, offsets, shift=1, conditions=False)


@pytest.mark.parametrize("k", (31, 47))
def test_ragged_block_sized_reads(ctx, orc, k):
    """reads on either side of the size that gets a whole block (8192 windows), among short ones"""
    rng = np.random.default_rng(7900 + k)
    lens = np.concatenate([[8192 + k - 1, 8192 + k, 9000, 300], rng.integers(50, 201, 70)]).astype(np.int64)
    rng.shuffle(lens)
    n = len(lens)
    a, b, offsets, protect = _ragged_batches(rng, lens, k)
    table, win = _table_for(orc, a, b, n, 0, k, offsets, protect_reads=protect)
    _check(ctx, table, win, b, n, 0, k, offsets, solid_mins=(1, 0))


# ---------------------------------------------------------------- counts that try the select
@pytest.mark.parametrize("k", (31, 47))
def test_counts_that_try_the_select(ctx, orc, k):
    rng = np.random.default_rng(8000 + k)
    n, L = 257, 150
    a, b = _uniform_batches(rng, n, L)
    (tk, tc), win = _table_for(orc, a, b, n, L, k)
    wild = rng.integers(1, 2**63, len(tk), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, len(tk), dtype=np.uint64)
    wild[::5] |= np.uint64(1 << 63)
    wild[::7] = np.uint64(U64_MAX)
    assert (wild >= np.uint64(1 << 63)).any() and (wild < np.uint64(1 << 63)).any() and (wild != 0).all()
    _check(ctx, (tk, wild), win, b, n, L, k, solid_mins=(1, 2**63, U64_MAX))
    _check(ctx, (tk, np.full(len(tk), 7, np.uint64)), win, b, n, L, k, solid_mins=(1, 7, 8))          # all counts equal
    _check(ctx, (tk, rng.integers(1, 3, len(tk)).astype(np.uint64)), win, b, n, L, k, solid_mins=(1, 2))    # counts in {1, 2}
    _check(ctx, (tk, rng.integers(1, 1000, len(tk)).astype(np.uint64)), win, b, n, L, k, solid_mins=(1, 500))
    # the same on long reads (the select that streams)
    n, L = 12, 1000
    a, b = _uniform_batches(rng, n, L)
    (tk, tc), win = _table_for(orc, a, b, n, L, k)
    wild = rng.integers(1, 2**63, len(tk), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    wild[::7] = np.uint64(U64_MAX)
    _check(ctx, (tk, wild), win, b, n, L, k, solid_mins=(1, 2**63))
    _check(ctx, (tk, rng.integers(1, 3, len(tk)).astype(np.uint64)), win, b, n, L, k, solid_mins=(1, 2))


# ---------------------------------------------------------------- solid_min and the span
@pytest.mark.parametrize("k", (31, 47))
def test_solid_min_values(ctx, orc, k):
    rng = np.random.default_rng(8100 + k)
    n, L = 257, 150
    a, b = _uniform_batches(rng, n, L)
    (tk, tc), win = _table_for(orc, a, b, n, L, k)
    tc = rng.integers(1, 4, len(tk)).astype(np.uint64)
    tc[::11] = np.uint64(1 << 63)
    tc[::13] = np.uint64(U64_MAX)
    _check(ctx, (tk, tc), win, b, n, L, k, solid_mins=(1, 0, 2, 2**63, U64_MAX))


def _runs_by_invalid_bytes(rng, L, k, bad_windows):
    """a read whose windows are valid except `bad_windows` (each made invalid by an N at its first base, which also takes the k - 1
    windows before it)"""
    r = random_reads(rng, L)
    for w in bad_windows:
        r[w] = ord("N")
    return r


def test_span_ties_and_boundaries(ctx, orc):
    """runs placed by hand: solid_min = 0 makes `solid` the same as `valid`, so N bytes draw the runs"""
    rng = np.random.default_rng(8200)
    k = 5
    empty = (np.zeros(0, np.uint64), np.zeros(0, np.uint64))

    def run(reads, L):
        n = len(reads)
        host = np.concatenate(reads)
        q, qf = orc_windows(orc, host, n, L, k)
        wo = orc.win_offsets_for(n, L, k, None)
        return _check(ctx, empty, (q, qf, wo), host, n, L, k, solid_mins=(0,), conditions=False)

    # W = 45 windows, windows 20 .. 24 invalid: two runs of 20, the earlier one is reported
    e = run([_runs_by_invalid_bytes(rng, 49, k, [24]), random_reads(rng, 49)], 49)
    assert int(e[0, 7]) == (20 << 32) | 0 and int(e[1, 7]) == (45 << 32) | 0
    # the later run longer by one: it wins
    e = run([_runs_by_invalid_bytes(rng, 50, k, [24])], 50)
    assert int(e[0, 7]) == (21 << 32) | 25
    # W = 256 (one wave, four registers per lane): a run over lanes 63 -> 64 and one of equal length over 127 -> 128 -> the first
    L = 256 + k - 1
    e = run([_runs_by_invalid_bytes(rng, L, k, [4, 44, 89, 134, 179, 224])], L)      # runs 5..39, 45..84 (40), 90..129 (40), ...
    assert int(e[0, 7]) == (40 << 32) | 45 and int(e[0, 0]) == 256 - 30
    e = run([_runs_by_invalid_bytes(rng, L, k, [9, 39, 99, 130, 190, 250])], L)    # runs 10..34, 40..94 (55), 100..125, 131..185 (55)
    assert int(e[0, 7]) == (55 << 32) | 40
    # a long read (one wave, 64 windows per step): the longest run crosses windows 255 -> 256 -> 257, an equal one comes later
    L = 1000
    e = run([_runs_by_invalid_bytes(rng, L, k, [99, 199, 305, 411, 500])], L)          # the last run, 501..995, is the longest
    assert int(e[0, 7]) == (495 << 32) | 501
    e = run([_runs_by_invalid_bytes(rng, L, k, [99, 199, 305, 411, 500, 600, 700, 800, 900])], L)   # 200..300 (101), 306..406 (101)
    assert int(e[0, 7]) == (101 << 32) | 200
    # a block-sized read: a run across the waves of a step and across steps
    L = 9000
    bad = list(range(4, 9000 - k, 100))
    bad.remove(304)                                                                # windows 205 .. 399 in one run
    e = run([_runs_by_invalid_bytes(rng, L, k, bad)], L)
    assert int(e[0, 7]) == (195 << 32) | 205


# ---------------------------------------------------------------- empty table, membership
@pytest.mark.parametrize("k", (31, 47))
def test_empty_table_and_membership(ctx, orc, k):
    rng = np.random.default_rng(8300 + k)
    n, L = 257, 150
    a, b = _uniform_batches(rng, n, L)
    b.reshape(n, L)[5, 70] = ord("N")
    table, win = _table_for(orc, a, b, n, L, k)
    _check(ctx, (table[0], None), win, b, n, L, k, solid_mins=(1, 2, 0))            # counts=None: 1 / 0
    q, qf, wo = win
    f = ctx.count_read_stats if k <= 31 else ctx.count_read_stats2
    bases = ctx.to_device(b)
    for sm in (1, 0):                                                              # n == 0, null pointers
        got = u64(f(bases, n, L, k, None, None, solid_min=sm))
        expect = _host_stats(np.zeros(len(q), np.uint64), qf, wo, sm)
        assert (got == expect).all(), sm
        assert (got[:, 1] == 0).all() and (got[:, 3:7] == 0).all() and (got[:, 0] > 0).all()
        if sm:
            assert (got[:, 1:] == 0).all()
        else:
            assert (got[:, 2] == got[:, 0]).all() and int(got[0, 7]) == (L - k + 1) << 32


# ---------------------------------------------------------------- at a size the oracle does not reach
@pytest.mark.parametrize("k", (31, 47))
def test_against_the_pinned_composition_at_size(ctx, k):
    import torch

    n, L = 100_000, 150
    W = L - k + 1
    a = ctx.gen_reads(n * L, seed=0xA11CE + k)
    b = ctx.gen_reads(n * L, seed=0xB0B + k)
    b.view(n, L)[::2] = a.view(n, L)[::2]
    g = torch.Generator(device=ctx.device).manual_seed(k)
    rows = torch.nonzero(torch.rand(n, device=ctx.device, generator=g) < 0.02).flatten()
    pos = torch.randint(0, L, (rows.numel(),), device=ctx.device, generator=g)
    b[rows * L + pos] = ord("N")
    one = k <= 31
    km, cnt = (ctx.count_canonical if one else ctx.count_canonical2)(a, n, L, k)
    per_window = u64((ctx.count_lookup_reads if one else ctx.count_lookup_reads2)(b, n, L, k, km, cnt))
    flags = (ctx.canonical_windows(b, n, L, k, want=("flags",)) if one else ctx.canonical_windows2(b, n, L, k))["flags"].cpu().numpy()
    wo = np.arange(n + 1, dtype=np.uint64) * np.uint64(W)
    for sm in (1, 2):
        expect = _dense_stats(per_window, flags, n, W, sm)
        got = u64(_call(ctx, k, b, n, L, km, cnt, sm))
        assert (got == expect).all(), (k, sm)
        if sm == 1:
            _assert_input(expect, per_window, flags, wo)


# ---------------------------------------------------------------- work buffer, determinism, arguments
@pytest.mark.parametrize("k", (31, 47))
def test_work_buffer_cap(ctx, orc, k):
    import torch

    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    rng = np.random.default_rng(8400 + k)
    n, L = 4000, 150
    a, b = _uniform_batches(rng, n, L)
    (tk, tc), (q, qf, wo) = _table_for(orc, a, b, n, L, k)
    d_tk, d_tc, bases = ctx.to_device(tk), ctx.to_device(tc), ctx.to_device(b)
    n_win = n * (L - k + 1)
    a256 = lambda x: (x + 255) & ~255
    # the documented working set (kmx.h): 8 + 1 bytes per window, two-word keys 16 more, each array rounded up to 256
    need = a256(8 * n_win) + a256(n_win) + (a256(16 * n_win) if k > 31 else 0)
    fn = ctx.lib.kmx_count_read_stats if k <= 31 else ctx.lib.kmx_count_read_stats2
    r = _lib.Reads(_ptr(bases), n, L, None)
    out = torch.full((8 * n,), POISON, dtype=torch.int64, device=ctx.device)
    try:
        ctx.set_work_buffer_limit(need - 1)
        allocs0 = ctx.work_buffer_info()[1]
        assert fn(ctx._h, C.byref(r), k, _ptr(d_tk), _ptr(d_tc), len(tc), 1, _ptr(out)) == _lib.E_NOMEM
        assert ctx.work_buffer_info()[1] == allocs0          # refused before the buffer was touched: nothing ran
        ctx.synchronize()
        assert (out == POISON).all()
        ctx.set_work_buffer_limit(need)                      # exactly the documented size: served (without a directory)
        assert fn(ctx._h, C.byref(r), k, _ptr(d_tk), _ptr(d_tc), len(tc), 1, _ptr(out)) == _lib.OK
        expect = _host_stats(host_lookup(tk, tc, q, qf), qf, wo, 1)
        assert (u64(out).reshape(n, 8) == expect).all()
    finally:
        ctx.set_work_buffer_limit(0)


@pytest.mark.parametrize("k", (31, 47))
def test_determinism_and_out_reuse(ctx, orc, k):
    import torch

    rng = np.random.default_rng(8500 + k)
    n, L = 500, 150
    out = torch.full((8 * n,), POISON, dtype=torch.int64, device=ctx.device)
    for _ in range(2):                                       # two batches through the same `out`
        a, b = _uniform_batches(rng, n, L)
        (tk, tc), (q, qf, wo) = _table_for(orc, a, b, n, L, k)
        d_tk, d_tc, bases = ctx.to_device(tk), ctx.to_device(tc), ctx.to_device(b)
        expect = _host_stats(host_lookup(tk, tc, q, qf), qf, wo, 1)
        got = _call(ctx, k, bases, n, L, d_tk, d_tc, 1, out=out)
        assert got.data_ptr() == out.data_ptr()
        first = u64(got).copy()
        assert (first == expect).all()
        again = u64(_call(ctx, k, bases, n, L, d_tk, d_tc, 1))
        assert first.tobytes() == again.tobytes()


def test_argument_errors(ctx):
    import torch

    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    rng = np.random.default_rng(86)
    n, L = 16, 150
    bases = ctx.to_device(random_reads(rng, n * L))
    keys = ctx.to_device(np.arange(1, 2001, dtype=np.uint64))     # a sorted table either way: 1000 two-word keys, or 2000 one-word
    cnts = ctx.to_device(np.ones(2000, np.uint64))
    out = torch.zeros(8 * n, dtype=torch.int64, device=ctx.device)
    r = _lib.Reads(_ptr(bases), n, L, None)
    lib, h = ctx.lib, ctx._h
    one, two = lib.kmx_count_read_stats, lib.kmx_count_read_stats2
    for k in (0, 32, 65):
        assert one(h, C.byref(r), k, _ptr(keys), _ptr(cnts), 1000, 2, _ptr(out)) == _lib.E_K_RANGE
        assert two(h, C.byref(r), k, _ptr(keys), _ptr(cnts), 1000, 2, _ptr(out)) == _lib.E_K_RANGE
    assert one(h, C.byref(r), 33, _ptr(keys), _ptr(cnts), 1000, 2, _ptr(out)) == _lib.E_K_RANGE
    assert two(h, C.byref(r), 31, _ptr(keys), _ptr(cnts), 1000, 2, _ptr(out)) == _lib.E_K_RANGE
    assert two(h, C.byref(r), 47, _ptr(keys[1:]), _ptr(cnts), 999, 2, _ptr(out)) == _lib.E_ARG      # misaligned two-word table
    assert one(h, C.byref(r), 31, _ptr(keys), _ptr(cnts), 1000, 2, None) == _lib.E_ARG              # d_stats NULL
    assert two(h, C.byref(r), 47, _ptr(keys), _ptr(cnts), 1000, 2, None) == _lib.E_ARG
    assert one(h, C.byref(r), 31, None, _ptr(cnts), 1000, 2, _ptr(out)) == _lib.E_ARG               # n > 0 without keys
    assert one(h, C.byref(r), 31, _ptr(keys), _ptr(cnts), 2**40 + 1, 2, _ptr(out)) == _lib.E_ARG
    empty = _lib.Reads(_ptr(bases), 0, L, None)
    assert one(h, C.byref(empty), 31, _ptr(keys), _ptr(cnts), 1000, 2, None) == _lib.OK             # n_reads == 0: a no-op
