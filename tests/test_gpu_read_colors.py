"""Per-read colour sets against a coloured table on the GPU: kmx_count_read_colors(2) (kmx_count_color.hip).

Every comparison is u64 equality of the whole (n_reads, 8) array and u32 equality of the whole (n_reads, n_colors) hit counts -- guard
words around both included, poison in them before the call -- against tests/color_np.py, the rule of kmx.h as a plain host loop (pinned
on strings in tests/test_color_np.py).  Inputs are made here: six samples cut from overlapping stretches of one random genome, either
strand, each with a private tail; their colours sit at bits 0, 3, 6, 31, 32 and 63, so that n_colors = 1, 7, 32, 33 and 64 see one,
three, four, five and six of them and every table has masks with bits at or above a smaller n_colors -- a window whose only colours
lie above the bound is no hit.  Of every seven reads one is cut from the genome (it crosses the stretches' ends: the mask switches),
one from a sample, one is a chimera of two samples, one is random (no hit), one has an N and mixed case, one is lower case, one has a
'>'.  At k = 1 there are two canonical 1-mers and no random read misses both: the table gives A / T the colours {0, 3} and C / G the
colours {3, 63}, and the read without a hit is all N.  Every table-driven test asserts of its own input, over its calls, that it holds
a read with ALL != ANY, one with N_SWITCH > 0, one without a hit, and one whose THRESH differs from both ALL and ANY."""
import ctypes as C

import numpy as np
import pytest

from tests.color_np import RC_ALL, RC_ANY, RC_N_HIT, RC_N_SWITCH, RC_N_VALID, RC_THRESH, interesting, read_colors
from tests.correct_np import count_kmers, dict_count, revcomp_bytes, table_arrays
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import random_reads, u64

pytestmark = pytest.mark.gpu

POISON = -0x5A5A5A5A5A5A5A5B
POISON32 = -0x5A5A5A5B
GUARD = 16
BITS = (0, 3, 6, 31, 32, 63)
COLORS = (64, 7, 33, 32, 1)
THRESHOLDS = ((1, 2), (0, 1), (2, 3), (1, 1))


class Source:
    def __init__(self, rng, k, size=1500):
        self.k = k
        self.genome = random_reads(rng, size)
        self.seqs = []
        self.table = {}
        for i, bit in enumerate(BITS):
            a = int(rng.integers(0, size // 2))
            s = np.concatenate([self.genome[a:a + int(rng.integers(size // 8, size // 2))], random_reads(rng, 2 * k + 20)])
            if i % 2:
                s = revcomp_bytes(s).copy()
            self.seqs.append(s)
            if k > 1:
                for key in count_kmers(s, 1, len(s), k):
                    self.table[key] = self.table.get(key, 0) | (1 << bit)
        if k == 1:
            self.table = {0: (1 << 0) | (1 << 3), 1: (1 << 3) | (1 << 63)}

    def _piece(self, rng, q, L):
        a = int(rng.integers(0, max(len(q) - L, 0) + 1))
        return np.resize(q[a:a + L], L).copy()

    def reads(self, rng, lens):
        out = []
        for r, L in enumerate(lens):
            L = int(L)
            kind = r % 7
            if L == 0:
                out.append(np.zeros(0, np.uint8))
                continue
            if kind == 0:
                s = self._piece(rng, self.genome, L)
            elif kind == 2:
                q, p = self.seqs[r % 6], self.seqs[(r + 1) % 6]
                s = np.resize(np.concatenate([q[len(q) - (L + 1) // 2:], p[:L // 2 + 1]]), L).copy()
            elif kind == 3:
                s = random_reads(rng, L) if self.k >= 11 else np.full(L, ord("N"), np.uint8)
            else:
                s = self._piece(rng, self.seqs[(r // 7) % 6], L)
            if kind == 4:
                s[int(rng.integers(0, L))] = ord("N")
                s[rng.random(L) < 0.3] |= 0x20
            elif kind == 5:
                s |= 0x20
            elif kind == 6:
                s[int(rng.integers(0, L))] = ord(">")
            out.append(s)
        return np.concatenate(out) if out else np.zeros(0, np.uint8)


class Tally:
    """what a table-driven test asks of its own input, gathered over its calls"""

    def __init__(self):
        self.seen = {}

    def add(self, rows):
        for key, v in interesting(rows).items():
            self.seen[key] = self.seen.get(key, False) or v

    def check(self):
        assert len(self.seen) == 4 and all(self.seen.values()), self.seen


def _device_table(ctx, table, k):
    tk, tc = table_arrays(table, k)
    return (ctx.to_device(tk), ctx.to_device(tc)) if len(tk) else (None, None)


def _check(ctx, k, host, n, L, table, n_colors, thr=(1, 2), offsets=None, shift=0, want_hits=True, tally=None, dev=None, expected=None):
    """one call against the host loop (or what it gave, `expected`): the whole guarded row array and the whole guarded hit counts"""
    import torch

    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    rows, hits = expected or read_colors(host, n, L, k, dict_count(table), n_colors, thr, offsets)
    d_tk, d_tc = dev if dev is not None else _device_table(ctx, table, k)
    buf = ctx.to_device(np.concatenate([np.zeros(shift, np.uint8), host, np.zeros(16, np.uint8)]))
    bases = buf[shift:shift + len(host)]
    d_off = None if offsets is None else ctx.to_device(np.asarray(offsets, np.uint64))
    wrows = torch.full((2 * GUARD + 8 * n,), POISON, dtype=torch.int64, device=ctx.device)
    whits = torch.full((2 * GUARD + n_colors * n,), POISON32, dtype=torch.int32, device=ctx.device)
    fn = ctx.lib.kmx_count_read_colors if k <= 31 else ctx.lib.kmx_count_read_colors2
    r = ctx._reads(bases, n, L, d_off)
    st = fn(ctx._h, C.byref(r), k, _ptr(d_tk), _ptr(d_tc), len(table), n_colors, thr[0], thr[1], _ptr(wrows[GUARD:]),
            _ptr(whits[GUARD:]) if want_hits else None)
    assert st == _lib.OK, st
    ctx.synchronize()
    want = np.full(len(wrows), POISON, np.int64).view(np.uint64)
    want[GUARD:GUARD + 8 * n] = rows.reshape(-1)
    g = u64(wrows)
    bad = np.nonzero(g != want)[0]
    assert len(bad) == 0, (k, L, n, n_colors, thr, shift, (bad[:8] - GUARD) // 8, (bad[:8] - GUARD) % 8, g[bad[:8]], want[bad[:8]])
    wanth = np.full(len(whits), POISON32, np.int32).view(np.uint32)
    if want_hits:
        wanth[GUARD:GUARD + n_colors * n] = hits.reshape(-1)
    gh = whits.cpu().numpy().view(np.uint32)
    badh = np.nonzero(gh != wanth)[0]
    assert len(badh) == 0, (k, L, n, n_colors, (badh[:8] - GUARD) // n_colors, gh[badh[:8]], wanth[badh[:8]])
    if tally is not None:
        tally.add(rows)
    return rows, hits


# ---------------------------------------------------------------- uniform reads
@pytest.mark.parametrize("k", (1, 15, 31, 33, 64))
def test_uniform(ctx, k):
    """one window, two, and both sides of one and of two steps of 64 windows; L = 150; d_bases at an odd address every other call"""
    rng = np.random.default_rng(9100 + k)
    src = Source(rng, k)
    dev = _device_table(ctx, src.table, k)
    tally = Tally()
    n = 28
    lengths = sorted({k - 1 + w for w in (1, 2, 63, 64, 65, 127, 128, 129)} | ({150} if k <= 150 else set()))
    for i, L in enumerate(lengths):
        host = src.reads(rng, [L] * n)
        for j in range(2):
            _check(ctx, k, host, n, L, src.table, COLORS[(i + 2 * j) % 5], THRESHOLDS[(i + j) % 4], shift=(i + j) % 2, tally=tally, dev=dev)
    tally.check()


# ---------------------------------------------------------------- ragged reads
def _ragged_lens(rng, k, hi, n_random=120):
    special = [0, 0, 1, k - 1, k, k, k + 1, 63, 64, 65, 127, 128, 129, 150, 300, k + 62, k + 63, k + 64]
    lens = np.concatenate([[x for x in special if x <= max(hi, k + 1)], rng.integers(0, min(hi, 300) + 1, n_random)]).astype(np.int64)
    rng.shuffle(lens)
    return lens


@pytest.mark.parametrize("k", (15, 47))
@pytest.mark.parametrize("bound", (0, 160, 256, 5000))
def test_ragged(ctx, k, bound):
    """lengths 0 .. 300 mixed (bound 160: up to 160), empty reads, reads shorter than k and of exactly k; offsets[0] != 0; a bound above
    256 takes the segment route and brings a read of about 5 000 bases"""
    rng = np.random.default_rng(9200 + k + bound)
    src = Source(rng, k, size=6000 if bound > 256 else 1500)
    lens = _ragged_lens(rng, k, bound if bound in (160, 256) else 300)
    if bound > 256:
        lens = np.concatenate([lens, [4987]])    # (its place in the batch makes it a cut from the genome: many switches)
        rng.shuffle(lens)
        at = int(np.nonzero(lens == 4987)[0][0])
        lens[0], lens[at] = lens[at], lens[0]
    n = len(lens)
    body = src.reads(rng, lens)
    lead = 37
    host = np.concatenate([random_reads(rng, lead), body, random_reads(rng, 11)])
    offsets = (lead + np.concatenate([[0], np.cumsum(lens)])).astype(np.uint64)
    tally = Tally()
    dev = _device_table(ctx, src.table, k)
    _check(ctx, k, host, n, bound, src.table, 64, (1, 2), offsets=offsets, tally=tally, dev=dev)
    _check(ctx, k, host, n, bound, src.table, 33, (2, 3), offsets=offsets, shift=1, tally=tally, dev=dev)       # the misaligned route
    _check(ctx, k, host, n, bound, src.table, 7, (1, 1), offsets=offsets, want_hits=False, tally=tally, dev=dev)
    tally.check()


# ---------------------------------------------------------------- more reads than four sweeps of the grid
def test_more_reads_than_four_sweeps(ctx):
    """the launch caps its grid at 16 blocks of four waves per CU (kmx_count_color.hip: RC_BLOCKS_PER_CU): 70 000 reads are more than
    4.2 sweeps of a 256-CU device, so every wave takes several reads"""
    import torch

    k, L, n, distinct = 15, 40, 70_000, 2000
    assert n > 4 * 4 * 16 * torch.cuda.get_device_properties(ctx.device).multi_processor_count
    rng = np.random.default_rng(9300)
    src = Source(rng, k)
    some = src.reads(rng, [L] * distinct)
    # reads are reduced one by one: the batch is the 2 000 reads 35 times over, and so is what the host loop says of them
    rows, hits = read_colors(some, distinct, L, k, dict_count(src.table), 64, (1, 2))
    tally = Tally()
    _check(ctx, k, np.tile(some, n // distinct), n, L, src.table, 64, (1, 2), tally=tally,
           expected=(np.tile(rows, (n // distinct, 1)), np.tile(hits, (n // distinct, 1))))
    tally.check()


# ---------------------------------------------------------------- where a pair of N_SWITCH may lie
@pytest.mark.parametrize("k", (15, 47))
def test_switch_across_a_step_and_not_across_reads(ctx, k):
    """windows 0 .. 63 of a stretch X belong to colour 0 alone and windows 64 .. to colour 3 alone.  Read as one read, the masks differ
    exactly between window positions 63 and 64 -- lanes 63 and 0 of two steps: one switch.  Cut into two reads there, the last window
    of the first and the first of the second are neighbours in the arrays and no pair: no switch"""
    rng = np.random.default_rng(9400 + k)
    X = random_reads(rng, 128 + k - 1)
    table = {}
    for bit, (a, b) in ((0, (0, 64)), (3, (64, 128))):
        for key in count_kmers(X[a:b + k - 1], 1, b - a + k - 1, k):
            assert key not in table
            table[key] = (1 << bit) | (1 << 63)
    rows, _ = _check(ctx, k, X, 1, len(X), table, 7)
    assert rows[0].tolist() == [128, 128, 128, 0, 9, 9, (64 << 32) | 0, 1]
    rows, _ = _check(ctx, k, X, 1, len(X), table, 64)           # with colour 63 in both halves: ALL = colour 63, still one switch
    assert rows[0].tolist() == [128, 128, 0, 1 << 63, 9 | (1 << 63), 9 | (1 << 63), (128 << 32) | 63, 1]
    L = 64 + k - 1
    two = np.concatenate([X[:L], X[64:64 + L]])
    rows, hits = _check(ctx, k, two, 2, L, table, 7)
    assert rows[:, RC_N_SWITCH].tolist() == [0, 0] and rows[:, RC_ALL].tolist() == [1, 8] and hits[:, [0, 3]].tolist() == [[64, 0], [0, 64]]
    offsets = np.array([0, L, 2 * L], np.uint64)
    rows, _ = _check(ctx, k, two, 2, 0, table, 7, offsets=offsets)
    assert rows[:, RC_N_SWITCH].tolist() == [0, 0]
    # the same table, a read that leaves X's first half one window early: the absent window separates
    Y = np.concatenate([X[:63 + k - 1], random_reads(rng, 1), X[64 + k:]])
    rows, _ = _check(ctx, k, Y, 1, len(Y), table, 7)
    assert int(rows[0, RC_N_SWITCH]) == 0 and int(rows[0, RC_N_HIT]) < int(rows[0, RC_N_VALID])


# ---------------------------------------------------------------- options and degenerate inputs
@pytest.mark.parametrize("k", (15, 47))
def test_thresholds_hits_and_tables(ctx, k):
    rng = np.random.default_rng(9500 + k)
    src = Source(rng, k)
    n, L = 70, 150
    host = src.reads(rng, [L] * n)
    dev = _device_table(ctx, src.table, k)
    tally = Tally()
    by_thr = {}
    for thr in THRESHOLDS:
        by_thr[thr], _ = _check(ctx, k, host, n, L, src.table, 64, thr, tally=tally, dev=dev)
        _check(ctx, k, host, n, L, src.table, 33, thr, want_hits=False, dev=dev)          # d_hits NULL: the rows all the same
    tally.check()
    base = by_thr[(1, 2)]
    assert (by_thr[(0, 1)][:, RC_THRESH] == base[:, RC_ANY]).all()
    every = base[:, RC_N_HIT] == base[:, RC_N_VALID]
    assert every.any() and (~every).any()
    assert (by_thr[(1, 1)][every, RC_THRESH] == base[every, RC_ALL]).all() and (by_thr[(1, 1)][~every, RC_THRESH] == 0).all()
    for nc in (1, 7, 32):
        _check(ctx, k, host, n, L, src.table, nc, (1, 2), dev=dev)
    # a table with every k-mer of the reads (random masks, none empty): every valid window is a hit
    full = {key: int(rng.integers(1, 2**63)) | (int(rng.integers(0, 2)) << 63) for key in count_kmers(host, n, L, k)}
    rows, _ = _check(ctx, k, host, n, L, full, 64, (1, 2))
    assert (rows[:, RC_N_HIT] == rows[:, RC_N_VALID]).all() and rows[:, RC_N_SWITCH].any()
    _check(ctx, k, host, n, L, full, 7, (2, 3))
    # an empty table: N_VALID is counted, everything else is zero
    rows, hits = _check(ctx, k, host, n, L, {}, 64, (0, 1))
    assert rows[:, RC_N_VALID].any() and (rows[:, 1:] == 0).all() and (hits == 0).all()
    # uniform reads shorter than k: rows and hit counts of zeros -- and written
    rows, hits = _check(ctx, k, host[:n * (k - 1)], n, k - 1, src.table, 33, dev=dev)
    assert (rows == 0).all() and (hits == 0).all()
    # ragged reads none of which has a window
    offsets = (np.arange(n + 1) * (k - 1)).astype(np.uint64)
    _check(ctx, k, host[:n * (k - 1)], n, 0, src.table, 33, offsets=offsets, dev=dev)


# ---------------------------------------------------------------- both search routes
def _dir_bytes(n, k):
    p = 0
    while p < 28 and p < 2 * k and (n >> p) > 8:
        p += 1
    return (4 * ((1 << p) + 1) + 255) & ~255


@pytest.mark.parametrize("k", (31, 47))
def test_both_search_routes(ctx, k):
    """a batch too small against its table for the lookup's directory to pay, and one large enough, each on a fresh context; which
    route ran shows in what the fresh context's work buffer holds: the documented arrays, or those and the directory.  Then the large
    batch again on the warm context"""
    from kmers_amd.api import Context

    rng = np.random.default_rng(9600 + k)
    src = Source(rng, k, size=12000)
    L = 100
    W = L - k + 1
    words = 1 if k <= 31 else 2
    a256 = lambda x: (x + 255) & ~255
    big = src.reads(rng, [L] * 600)
    n_table = len(src.table)
    tally = Tally()
    for n, with_dir in ((1, False), (600, True)):
        assert (n * W >= words * n_table // 64) == with_dir and n_table > 8
        c = Context()
        try:
            _check(c, k, big[:n * L], n, L, src.table, 64, (1, 2), tally=tally)
            arrays = a256(8 * n * W) + a256(n * W) + (a256(16 * n * W) if words == 2 else 0)
            assert c.work_buffer_info()[0] == arrays + (_dir_bytes(n_table, k) if with_dir else 0)
            if with_dir:
                _check(c, k, big[:n * L], n, L, src.table, 33, (2, 3), tally=tally)
        finally:
            c.close()
    tally.check()


# ---------------------------------------------------------------- errors
def test_argument_errors(ctx):
    import torch

    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    rng = np.random.default_rng(97)
    n, L = 16, 150
    bases = ctx.to_device(random_reads(rng, n * L))
    keys = ctx.to_device(np.arange(1, 2001, dtype=np.uint64))     # a sorted table either way: 1000 two-word keys, or 2000 one-word
    cols = ctx.to_device(np.ones(2000, np.uint64))
    rows = torch.full((8 * n,), POISON, dtype=torch.int64, device=ctx.device)
    hits = torch.full((64 * n,), POISON32, dtype=torch.int32, device=ctx.device)
    r = _lib.Reads(_ptr(bases), n, L, None)
    h = ctx._h
    one, two = ctx.lib.kmx_count_read_colors, ctx.lib.kmx_count_read_colors2
    for k in (0, 32, 65):
        assert one(h, C.byref(r), k, _ptr(keys), _ptr(cols), 1000, 8, 1, 2, _ptr(rows), _ptr(hits)) == _lib.E_K_RANGE
        assert two(h, C.byref(r), k, _ptr(keys), _ptr(cols), 1000, 8, 1, 2, _ptr(rows), _ptr(hits)) == _lib.E_K_RANGE
    assert one(h, C.byref(r), 33, _ptr(keys), _ptr(cols), 1000, 8, 1, 2, _ptr(rows), _ptr(hits)) == _lib.E_K_RANGE
    assert two(h, C.byref(r), 31, _ptr(keys), _ptr(cols), 1000, 8, 1, 2, _ptr(rows), _ptr(hits)) == _lib.E_K_RANGE
    for fn, k in ((one, 31), (two, 47)):
        for nc in (0, 65):
            assert fn(h, C.byref(r), k, _ptr(keys), _ptr(cols), 1000, nc, 1, 2, _ptr(rows), _ptr(hits)) == _lib.E_ARG
        assert fn(h, C.byref(r), k, _ptr(keys), _ptr(cols), 1000, 8, 1, 0, _ptr(rows), _ptr(hits)) == _lib.E_ARG        # thr_den == 0
        assert fn(h, C.byref(r), k, _ptr(keys), _ptr(cols), 1000, 8, 0, 0, _ptr(rows), _ptr(hits)) == _lib.E_ARG
        assert fn(h, C.byref(r), k, _ptr(keys), _ptr(cols), 1000, 8, 3, 2, _ptr(rows), _ptr(hits)) == _lib.E_ARG        # thr_num > thr_den
        assert fn(h, C.byref(r), k, _ptr(keys), None, 1000, 8, 1, 2, _ptr(rows), _ptr(hits)) == _lib.E_ARG              # membership has no colours
        assert fn(h, C.byref(r), k, None, _ptr(cols), 1000, 8, 1, 2, _ptr(rows), _ptr(hits)) == _lib.E_ARG              # n > 0 without keys
        assert fn(h, C.byref(r), k, _ptr(keys), _ptr(cols), 1000, 8, 1, 2, None, _ptr(hits)) == _lib.E_ARG              # d_rows NULL
        assert fn(h, C.byref(r), k, _ptr(keys), _ptr(cols), 2**40 + 1, 8, 1, 2, _ptr(rows), _ptr(hits)) == _lib.E_ARG
        assert fn(None, C.byref(r), k, _ptr(keys), _ptr(cols), 1000, 8, 1, 2, _ptr(rows), _ptr(hits)) == _lib.E_ARG
    assert two(h, C.byref(r), 47, _ptr(keys[1:]), _ptr(cols), 999, 8, 1, 2, _ptr(rows), _ptr(hits)) == _lib.E_ARG      # misaligned two-word table
    ctx.synchronize()
    assert (rows == POISON).all() and (hits == POISON32).all()                                                      # nothing was written
    empty = _lib.Reads(_ptr(bases), 0, L, None)
    assert one(h, C.byref(empty), 31, _ptr(keys), _ptr(cols), 1000, 8, 1, 2, None, None) == _lib.OK                   # n_reads == 0: a no-op
    assert one(h, C.byref(r), 31, None, None, 0, 8, 2, 2, _ptr(rows), _ptr(hits)) == _lib.OK                          # an empty table, NULL colours
    ctx.synchronize()
    assert (hits[:8 * n] == 0).all() and (hits[8 * n:] == POISON32).all()


def test_work_buffer_cap(ctx):
    import torch

    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    k = 31
    rng = np.random.default_rng(9800)
    src = Source(rng, k)
    n, L = 400, 150
    host = src.reads(rng, [L] * n)
    d_tk, d_tc = _device_table(ctx, src.table, k)
    bases = ctx.to_device(host)
    n_win = n * (L - k + 1)
    a256 = lambda x: (x + 255) & ~255
    need = a256(8 * n_win) + a256(n_win)      # the documented working set (kmx.h)
    r = _lib.Reads(_ptr(bases), n, L, None)
    rows = torch.full((8 * n,), POISON, dtype=torch.int64, device=ctx.device)
    hits = torch.full((64 * n,), POISON32, dtype=torch.int32, device=ctx.device)
    fn = ctx.lib.kmx_count_read_colors
    try:
        ctx.set_work_buffer_limit(need - 1)
        allocs0 = ctx.work_buffer_info()[1]
        assert fn(ctx._h, C.byref(r), k, _ptr(d_tk), _ptr(d_tc), len(src.table), 64, 1, 2, _ptr(rows), _ptr(hits)) == _lib.E_NOMEM
        assert ctx.work_buffer_info()[1] == allocs0          # refused before the buffer was touched: nothing ran
        ctx.synchronize()
        assert (rows == POISON).all() and (hits == POISON32).all()
        ctx.set_work_buffer_limit(need)                      # exactly the documented size: served (without a directory)
        assert fn(ctx._h, C.byref(r), k, _ptr(d_tk), _ptr(d_tc), len(src.table), 64, 1, 2, _ptr(rows), _ptr(hits)) == _lib.OK
        want, wh = read_colors(host, n, L, k, dict_count(src.table), 64, (1, 2))
        ctx.synchronize()
        assert (u64(rows).reshape(n, 8) == want).all() and (hits.cpu().numpy().view(np.uint32).reshape(n, 64) == wh).all()
    finally:
        ctx.set_work_buffer_limit(0)


# ---------------------------------------------------------------- the Python layer and determinism
@pytest.mark.parametrize("k", (15, 47))
def test_api_and_determinism(ctx, k):
    import torch

    rng = np.random.default_rng(9900 + k)
    src = Source(rng, k)
    lens = _ragged_lens(rng, k, 300)
    n = len(lens)
    host = src.reads(rng, lens)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    d_tk, d_tc = _device_table(ctx, src.table, k)
    bases, d_off = ctx.to_device(host), ctx.to_device(offsets)
    fn = ctx.count_read_colors if k <= 31 else ctx.count_read_colors2
    want, wh = read_colors(host, n, 0, k, dict_count(src.table), 33, (2, 3), offsets)
    a = fn(bases, n, 0, k, d_tk, d_tc, 33, threshold=(2, 3), offsets=d_off, hits=True)
    b = fn(bases, n, 0, k, d_tk, d_tc, 33, threshold=(2, 3), offsets=d_off, hits=True)
    assert a[0].shape == (n, 8) and a[1].shape == (n, 33) and a[1].dtype == torch.int32
    assert (u64(a[0]) == want).all() and (a[1].cpu().numpy().view(np.uint32) == wh).all()
    assert u64(a[0]).tobytes() == u64(b[0]).tobytes() and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()
    out = torch.full((8 * n,), POISON, dtype=torch.int64, device=ctx.device)
    rows, none = fn(bases, n, 0, k, d_tk, d_tc, 33, threshold=(2, 3), offsets=d_off, out=out)
    assert none is None and rows.data_ptr() == out.data_ptr() and (u64(rows) == want).all()
    half = fn(bases, n, 0, k, d_tk, d_tc, 33, offsets=d_off)[0]           # the default threshold: one half
    assert (u64(half) == read_colors(host, n, 0, k, dict_count(src.table), 33, (1, 2), offsets)[0]).all()
