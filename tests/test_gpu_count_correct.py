"""Substitution errors corrected against a count table on the GPU: kmx_count_correct_reads(2) (kmx_count_correct.hip).

Every comparison is byte equality of the whole output buffer -- guard bytes around it included, poison in it before the call -- and
u64 equality of the whole (n_reads, 4) array against tests/correct_np.py, the rule of kmx.h as a plain host loop (pinned on strings in
tests/test_correct_np.py).  Inputs are made here: reads cut from a random genome and from a variant of it that differs in single
bases, from both strands; the table holds the k-mers of both with counts 3 .. 9, and the k-mers the reads' errors make with
count 1 or 0.  Of every eight reads one is clean, one has an error at a position that matters (0, k - 1, 63, 64, L - k, L - 1), one two errors
less than k apart, one a third base at a site where genome and variant differ (two bases fix it), one is random, one has an error
and an N, one scattered errors in mixed case, one is lower case.  Every table-driven test asserts of its own input that it holds a
CORRECTED position, an AMBIGUOUS one, a candidate nothing fixes and a read without a candidate -- except at k = 1, where A / T and
C / G are one canonical 1-mer each: fixing bases come in pairs, so no position is ever CORRECTED, and with one of the two 1-mers solid
and the other weak (the only table with candidates AND fixing bases) every candidate has its pair: AMBIGUOUS, none left unfixed."""
import ctypes as C

import numpy as np
import pytest

from tests.correct_np import correct_reads, count_kmers, dict_count, revcomp_bytes, table_arrays
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import random_reads, u64

pytestmark = pytest.mark.gpu

POISON = 0xA5
GUARD = 64
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _other(c, step):
    return int(ACGT[(int(np.nonzero(ACGT == (c & 0xDF))[0][0]) + step) % 4])


class Source:
    """a genome, a variant of it that differs in one base every 53, and the table of both"""

    def __init__(self, rng, k, size=1500):
        self.k = k
        self.genome = random_reads(rng, size)
        self.variant = self.genome.copy()
        self.sites = np.arange(40, size - 40, 53)
        for s in self.sites:
            self.variant[s] = _other(self.variant[s], 1)
        self.table = {}
        if k <= 3:   # every k-mer there is: solid or weak at random, so that a weak base has one, two or no way out
            for key in count_kmers(random_reads(rng, 4000), 1, 4000, k):
                self.table[key] = 5 if rng.random() < 0.45 else 1
            if k == 1:
                self.table = {0: 5, 1: 1}   # A / T solid, C / G weak
        else:
            for seq in (self.genome, self.variant):
                for key in count_kmers(seq, 1, size, k):
                    self.table[key] = int(rng.integers(3, 10))

    def cut(self, rng, L, site=None):
        """L bases of the genome or the variant (over `site` when given), either strand -> (bases, position of the site or None,
        whether the bases are the reverse strand's)"""
        size = len(self.genome)
        if site is None:
            a = int(rng.integers(0, size - L + 1))
        else:
            a = int(rng.integers(max(0, site - L + 1), min(site, size - L) + 1))
        s = (self.variant if rng.random() < 0.5 else self.genome)[a:a + L].copy()
        at = None if site is None else site - a
        rev = rng.random() < 0.5
        if rev:
            s = revcomp_bytes(s).copy()
            at = None if at is None else L - 1 - at
        return s, at, rev

    def reads(self, rng, lens):
        """the eight kinds in turn; the k-mers their errors make go into the table as weak entries (count 1, some 0)"""
        k = self.k
        out = []
        for r, L in enumerate(lens):
            L = int(L)
            kind = r % 8
            if L == 0:
                out.append(np.zeros(0, np.uint8))
                continue
            site = int(self.sites[r % len(self.sites)]) if kind == 3 else None
            s, at, rev = self.cut(rng, L, site)
            marks = [p for p in (0, k - 1, 63, 64, L - k, L - 1) if 0 <= p < L]
            if kind == 1:
                p = marks[(r // 8) % len(marks)]
                s[p] = _other(s[p], 1 + r % 3)
            elif kind == 2 and L >= 2:
                p = int(rng.integers(0, L - 1))
                q = min(L - 1, p + 1 + int(rng.integers(0, max(k - 1, 1))))
                s[p], s[q] = _other(s[p], 1), _other(s[q], 2)
            elif kind == 3:
                g, v = int(self.genome[site]), int(self.variant[site])
                third = [int(c) for c in ACGT if c not in (g, v)][r % 2]
                s[at] = int(revcomp_bytes(bytes([third]))[0]) if rev else third   # (the reverse strand spells the complement)
            elif kind == 4:
                s = random_reads(rng, L)
            elif kind == 5:
                p = marks[(r // 8 + 1) % len(marks)]
                s[p] = _other(s[p], 2)
                s[int(rng.integers(0, L))] = ord("N") if r % 16 else ord(">")
            elif kind == 6:
                for p in np.nonzero(rng.random(L) < 0.02)[0]:
                    s[p] = _other(s[p], int(rng.integers(1, 4)))
                s[rng.random(L) < 0.3] |= 0x20
            elif kind == 7:
                s |= 0x20
            out.append(s)
        host = np.concatenate(out) if out else np.zeros(0, np.uint8)
        return host

    def add_weak(self, host, n, L, offsets=None):
        if self.k <= 3:
            return
        for i, key in enumerate(count_kmers(host, n, L, self.k, offsets)):
            if key not in self.table:
                self.table[key] = 0 if i % 7 == 0 else 1


class Tally:
    """what a table-driven test asks of its own input, gathered over its calls"""

    def __init__(self):
        self.corrected = self.ambiguous = self.unfixed = self.clean_reads = 0

    def add(self, rows, host, n, L, k, offsets):
        r = rows.astype(np.int64)
        self.corrected += int(r[:, 2].sum())
        self.ambiguous += int(r[:, 3].sum())
        self.unfixed += int((r[:, 1] - r[:, 2] - r[:, 3]).sum())
        lens = np.full(n, L) if offsets is None else np.diff(np.asarray(offsets).astype(np.int64))
        self.clean_reads += int(((r[:, 1] == 0) & (lens >= k)).sum())

    def check(self, k):
        assert self.ambiguous > 0 and self.clean_reads > 0, vars(self)
        if k == 1:
            assert self.corrected == 0 and self.unfixed == 0, vars(self)     # (what one table of 1-mers can hold: the module's docstring)
        else:
            assert self.corrected > 0 and self.unfixed > 0, vars(self)


def _fn(ctx, k):
    return ctx.count_correct_reads if k <= 31 else ctx.count_correct_reads2


def _device_table(ctx, table, k, counts=True):
    tk, tc = table_arrays(table, k)
    return (ctx.to_device(tk) if len(tk) else None), (ctx.to_device(tc) if counts and len(tk) else None)


def _check(ctx, k, host, n, L, table, solid_min, min_cover, offsets=None, shift=0, counts=True, tally=None, dev=None, expected=None):
    """one call against the host loop (or what it gave, `expected`): the whole guarded output buffer and the whole row array"""
    import torch

    expect, rows = expected or correct_reads(host, n, L, k, dict_count(table, membership=not counts), solid_min, min_cover, offsets)
    d_tk, d_tc = dev if dev is not None else _device_table(ctx, table, k, counts)
    buf = ctx.to_device(np.concatenate([np.zeros(shift, np.uint8), host, np.zeros(16, np.uint8)]))
    bases = buf[shift:shift + len(host)]
    d_off = None if offsets is None else ctx.to_device(np.asarray(offsets, np.uint64))
    whole = torch.full((GUARD + len(host) + GUARD,), POISON, dtype=torch.uint8, device=ctx.device)
    out = whole[GUARD:GUARD + len(host)]
    got_out, got_rows = _fn(ctx, k)(bases, n, L, k, d_tk, d_tc, solid_min=solid_min, min_cover=min_cover, offsets=d_off, out=out)
    assert got_out.data_ptr() == out.data_ptr()
    first, last = (0, n * L) if offsets is None else (int(offsets[0]), int(offsets[n]))
    want = np.full(len(whole), POISON, np.uint8)
    want[GUARD + first:GUARD + last] = expect[first:last]
    got = whole.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (k, L, n, solid_min, min_cover, shift, bad[:8] - GUARD, got[bad[:8]], want[bad[:8]])
    g = u64(got_rows)
    assert g.shape == rows.shape
    badr = np.nonzero((g != rows).any(axis=1))[0]
    assert len(badr) == 0, (k, L, n, solid_min, min_cover, badr[:5], g[badr[:3]], rows[badr[:3]])
    if tally is not None:
        tally.add(rows, host, n, L, k, offsets)
    return expect, rows


# ---------------------------------------------------------------- uniform reads
@pytest.mark.parametrize("k", (1, 2, 8, 15, 31, 33, 47, 64))
def test_uniform(ctx, k):
    """one window, the step boundaries of positions and of windows, the full 63-back history at k = 64; d_bases at an odd address"""
    rng = np.random.default_rng(9100 + k)
    src = Source(rng, k)
    tally = Tally()
    n = 96
    batches = []
    for L in sorted({L for L in (k, k + 1, 63, 64, 65, 127, 128, 129, 150) if L >= k}):
        host = src.reads(rng, [L] * n)
        src.add_weak(host, n, L)
        batches.append((L, host))
    dev = _device_table(ctx, src.table, k)
    for i, (L, host) in enumerate(batches):
        for mc in sorted({1, min(2, k), k}):
            _check(ctx, k, host, n, L, src.table, 3, mc, shift=(i + mc) % 2, tally=tally if mc == 1 else None, dev=dev)
    tally.check(k)


# ---------------------------------------------------------------- ragged reads
def _ragged_lens(rng, k, hi, n_random=150):
    special = [0, 0, 1, k - 1, k, k, k + 1, 63, 64, 65, 127, 128, 129, 150, 300]
    lens = np.concatenate([[x for x in special if x <= max(hi, k + 1)], rng.integers(0, min(hi, 300) + 1, n_random)]).astype(np.int64)
    rng.shuffle(lens)
    return lens


@pytest.mark.parametrize("k", (15, 31, 47))
@pytest.mark.parametrize("bound", (0, 160, 256, 5000))
def test_ragged(ctx, k, bound):
    """lengths 0 .. 300 mixed (bound 160: up to 160), empty reads, reads shorter than k and of exactly k; offsets[0] != 0; a bound above
    256 takes the segment route and brings a read of about 5 000 bases; the bytes before offsets[0] and behind offsets[n] stay poison"""
    rng = np.random.default_rng(9200 + k + bound)
    src = Source(rng, k, size=6000 if bound > 256 else 1500)
    lens = _ragged_lens(rng, k, bound if bound in (160, 256) else 300)
    if bound > 256:
        lens = np.concatenate([lens, [4987]])
        rng.shuffle(lens)
    n = len(lens)
    body = src.reads(rng, lens)
    lead = 37
    host = np.concatenate([random_reads(rng, lead), body, random_reads(rng, 11)])
    offsets = (lead + np.concatenate([[0], np.cumsum(lens)])).astype(np.uint64)
    src.add_weak(host, n, 0, offsets)
    tally = Tally()
    dev = _device_table(ctx, src.table, k)
    _check(ctx, k, host, n, bound, src.table, 3, 1, offsets=offsets, tally=tally, dev=dev)
    _check(ctx, k, host, n, bound, src.table, 3, 2, offsets=offsets, shift=1, dev=dev)       # the misaligned route
    tally.check(k)


# ---------------------------------------------------------------- more reads than one sweep of the grid
def test_more_reads_than_one_sweep(ctx):
    """the launch caps its grid at 16 blocks of four waves per CU (kmx_count_correct.hip: CR_BLOCKS_PER_CU): 70 000 reads are more
    than 4.2 sweeps of a 256-CU device, so every wave takes several reads"""
    import torch

    k, L, n, distinct = 15, 40, 70_000, 2000
    assert n > 4 * 16 * torch.cuda.get_device_properties(ctx.device).multi_processor_count
    rng = np.random.default_rng(9300)
    src = Source(rng, k)
    some = src.reads(rng, [L] * distinct)
    src.add_weak(some, distinct, L)
    # reads are decided one by one: the batch is the 2 000 reads 35 times over, and so is what the host loop says of them
    e, rows = correct_reads(some, distinct, L, k, dict_count(src.table), 3, 1)
    tally = Tally()
    _check(ctx, k, np.tile(some, n // distinct), n, L, src.table, 3, 1, tally=tally, expected=(np.tile(e, n // distinct), np.tile(rows, (n // distinct, 1))))
    tally.check(k)


# ---------------------------------------------------------------- both search routes
def _dir_bytes(n, k):
    p = 0
    while p < 28 and p < 2 * k and (n >> p) > 8:
        p += 1
    return (4 * ((1 << p) + 1) + 255) & ~255


@pytest.mark.parametrize("k", (31, 47))
def test_both_search_routes(ctx, k):
    """a batch too small against its table for the directory to pay (count_lookup_wants_dir: fewer windows than n / 64 per key word), and one
    large enough; which route ran shows in what a fresh context's work buffer holds: the documented arrays, or those and the directory"""
    from kmers_amd.api import Context

    rng = np.random.default_rng(9400 + k)
    src = Source(rng, k, size=12000)
    L = 100
    W = L - k + 1
    words = 1 if k <= 31 else 2
    a256 = lambda x: (x + 255) & ~255
    big = src.reads(rng, [L] * 600)
    src.add_weak(big, 600, L)
    n_table = len(src.table)
    tally = Tally()
    for n, with_dir in ((2, False), (600, True)):
        assert (n * W >= words * n_table // 64) == with_dir and n_table > 8
        c = Context()
        try:
            _check(c, k, big[:n * L], n, L, src.table, 3, 1, tally=tally)
            arrays = a256(8 * n * W) + a256(n * W) + (a256(16 * n * W) if words == 2 else 0)
            assert c.work_buffer_info()[0] == arrays + (_dir_bytes(n_table, k) if with_dir else 0)
        finally:
            c.close()
    tally.check(k)


# ---------------------------------------------------------------- options and degenerate inputs
@pytest.mark.parametrize("k", (15, 47))
def test_options_and_degenerate_inputs(ctx, k):
    import torch

    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    rng = np.random.default_rng(9500 + k)
    src = Source(rng, k)
    n, L = 120, 100
    host = src.reads(rng, [L] * n)
    src.add_weak(host, n, L)
    assert 0 in src.table.values()                                                  # entries with count 0: they read as absent
    tally = Tally()
    _check(ctx, k, host, n, L, src.table, 3, 1, tally=tally)
    tally.check(k)
    _check(ctx, k, host, n, L, src.table, 1, 1, counts=False)                         # d_counts = NULL: membership, count-0 entries are members
    e0, r0 = _check(ctx, k, host, n, L, src.table, 0, 1)                              # solid_min 0: no candidate
    assert (e0 == host).all() and (r0 == 0).all()
    _check(ctx, k, host, n, L, src.table, 1, 1)
    e9, r9 = _check(ctx, k, host, n, L, src.table, 10, 1)                             # above every count: all weak, nothing fixes
    assert (e9 == host).all() and (r9[:, 2:] == 0).all() and (r9[:, 1] > 0).all()
    ee, re_ = _check(ctx, k, host, n, L, {}, 1, 1)                                    # an empty table: the candidates are still counted
    assert (ee == host).all() and (re_[:, 2:] == 0).all() and (re_[:, 1] > 0).any() and (re_[:, 0] == r9[:, 0]).all()
    # d_fixes = NULL: the bytes all the same
    expect, _ = correct_reads(host, n, L, k, dict_count(src.table), 3, 1)
    d_tk, d_tc = _device_table(ctx, src.table, k)
    bases = ctx.to_device(host)
    out = torch.full((n * L,), POISON, dtype=torch.uint8, device=ctx.device)
    fn = ctx.lib.kmx_count_correct_reads if k <= 31 else ctx.lib.kmx_count_correct_reads2
    r = _lib.Reads(_ptr(bases), n, L, None)
    assert fn(ctx._h, C.byref(r), k, _ptr(d_tk), _ptr(d_tc), len(src.table), 3, 1, _ptr(out), None) == _lib.OK
    ctx.synchronize()
    assert (out.cpu().numpy() == expect).all()
    # uniform reads shorter than k: copied through, rows zero -- and written
    short = host[:n * (k - 1)]
    es, rs = _check(ctx, k, short, n, k - 1, src.table, 3, 1)
    assert (es == short).all() and (rs == 0).all()


@pytest.mark.parametrize("k", (31, 47))
def test_weak_column_is_read_stats(ctx, k):
    from kmers_amd import _lib

    rng = np.random.default_rng(9600 + k)
    src = Source(rng, k)
    n, L = 200, 150
    host = src.reads(rng, [L] * n)
    src.add_weak(host, n, L)
    d_tk, d_tc = _device_table(ctx, src.table, k)
    bases = ctx.to_device(host)
    stats = ctx.count_read_stats if k <= 31 else ctx.count_read_stats2
    for sm in (1, 3):
        _, rows = _fn(ctx, k)(bases, n, L, k, d_tk, d_tc, solid_min=sm, min_cover=1)
        rs = u64(stats(bases, n, L, k, d_tk, d_tc, solid_min=sm))
        weak = rs[:, _lib.RS_N_VALID] - rs[:, _lib.RS_N_SOLID]
        assert (u64(rows)[:, _lib.CR_N_WEAK] == weak).all() and weak.any()


@pytest.mark.parametrize("k", (15, 31, 47))
def test_clean_reads_come_back_unchanged(ctx, k):
    """reads cut from a genome without errors against their own table: zero candidates, the bytes as they were"""
    rng = np.random.default_rng(9700 + k)
    genome = random_reads(rng, 2000)
    n, L = 300, 100
    host = np.concatenate([genome[a:a + L] if r % 2 else revcomp_bytes(genome[a:a + L])
                           for r, a in enumerate(rng.integers(0, len(genome) - L + 1, n))])
    host[rng.random(len(host)) < 0.3] |= 0x20
    table = count_kmers(host, n, L, k)
    low = min(table.values())
    expect, rows = _check(ctx, k, host, n, L, table, low, 1)
    assert (expect == host).all() and (rows == 0).all()


# ---------------------------------------------------------------- errors
def test_argument_errors(ctx):
    import torch

    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    rng = np.random.default_rng(98)
    n, L = 16, 150
    buf = torch.full((2 * n * L,), POISON, dtype=torch.uint8, device=ctx.device)
    bases = buf[:n * L]
    bases.copy_(ctx.to_device(random_reads(rng, n * L)))
    out = buf[n * L:]
    keys = ctx.to_device(np.arange(1, 2001, dtype=np.uint64))     # a sorted table either way: 1000 two-word keys, or 2000 one-word
    cnts = ctx.to_device(np.ones(2000, np.uint64))
    fixes = torch.zeros(4 * n, dtype=torch.int64, device=ctx.device)
    r = _lib.Reads(_ptr(bases), n, L, None)
    lib, h = ctx.lib, ctx._h
    one, two = lib.kmx_count_correct_reads, lib.kmx_count_correct_reads2
    for k in (0, 32, 65):
        assert one(h, C.byref(r), k, _ptr(keys), _ptr(cnts), 1000, 2, 1, _ptr(out), _ptr(fixes)) == _lib.E_K_RANGE
        assert two(h, C.byref(r), k, _ptr(keys), _ptr(cnts), 1000, 2, 1, _ptr(out), _ptr(fixes)) == _lib.E_K_RANGE
    assert one(h, C.byref(r), 33, _ptr(keys), _ptr(cnts), 1000, 2, 1, _ptr(out), _ptr(fixes)) == _lib.E_K_RANGE
    assert two(h, C.byref(r), 31, _ptr(keys), _ptr(cnts), 1000, 2, 1, _ptr(out), _ptr(fixes)) == _lib.E_K_RANGE
    for fn, k in ((one, 31), (two, 47)):
        for mc in (0, k + 1):
            assert fn(h, C.byref(r), k, _ptr(keys), _ptr(cnts), 1000, 2, mc, _ptr(out), _ptr(fixes)) == _lib.E_ARG
        assert fn(h, C.byref(r), k, _ptr(keys), _ptr(cnts), 1000, 2, k, _ptr(out), _ptr(fixes)) == _lib.OK
        assert fn(h, C.byref(r), k, _ptr(keys), _ptr(cnts), 1000, 2, 1, None, _ptr(fixes)) == _lib.E_ARG           # d_out_bases NULL
        assert fn(h, C.byref(r), k, None, _ptr(cnts), 1000, 2, 1, _ptr(out), _ptr(fixes)) == _lib.E_ARG            # n > 0 without keys
        assert fn(h, C.byref(r), k, _ptr(keys), _ptr(cnts), 2**40 + 1, 2, 1, _ptr(out), _ptr(fixes)) == _lib.E_ARG
        # overlapping output: in place, by one byte at either end
        ctx.synchronize()
        before = buf.clone()
        for o in (bases, buf[1:1 + n * L], buf[n * L - 1:2 * n * L - 1]):
            assert fn(h, C.byref(r), k, _ptr(keys), _ptr(cnts), 1000, 2, 1, _ptr(o), _ptr(fixes)) == _lib.E_ARG
        ctx.synchronize()
        assert (buf == before).all()
    assert two(h, C.byref(r), 47, _ptr(keys[1:]), _ptr(cnts), 999, 2, 1, _ptr(out), _ptr(fixes)) == _lib.E_ARG      # misaligned two-word table
    empty = _lib.Reads(_ptr(bases), 0, L, None)
    assert one(h, C.byref(empty), 31, _ptr(keys), _ptr(cnts), 1000, 2, 1, None, None) == _lib.OK                   # n_reads == 0: a no-op
    # ragged reads: the written range is [offsets[0], offsets[n]); an output that overlaps the input only outside it is served
    offs = ctx.to_device(np.array([100, 250, 400], np.uint64))
    rr = _lib.Reads(_ptr(buf), 2, 0, _ptr(offs))
    assert one(h, C.byref(rr), 31, _ptr(keys), _ptr(cnts), 1000, 2, 1, _ptr(buf[200:]), None) == _lib.E_ARG
    assert one(h, C.byref(rr), 31, _ptr(keys), _ptr(cnts), 1000, 2, 1, _ptr(buf[300:]), None) == _lib.OK
    ctx.synchronize()


@pytest.mark.parametrize("k", (31, 47))
def test_work_buffer_cap(ctx, k):
    import torch

    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    rng = np.random.default_rng(9800 + k)
    src = Source(rng, k)
    n, L = 400, 150
    host = src.reads(rng, [L] * n)
    d_tk, d_tc = _device_table(ctx, src.table, k)
    bases = ctx.to_device(host)
    n_win = n * (L - k + 1)
    a256 = lambda x: (x + 255) & ~255
    need = a256(8 * n_win) + a256(n_win) + (a256(16 * n_win) if k > 31 else 0)      # the documented working set (kmx.h)
    fn = ctx.lib.kmx_count_correct_reads if k <= 31 else ctx.lib.kmx_count_correct_reads2
    r = _lib.Reads(_ptr(bases), n, L, None)
    out = torch.full((n * L,), POISON, dtype=torch.uint8, device=ctx.device)
    fixes = torch.full((4 * n,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=ctx.device)
    try:
        ctx.set_work_buffer_limit(need - 1)
        allocs0 = ctx.work_buffer_info()[1]
        assert fn(ctx._h, C.byref(r), k, _ptr(d_tk), _ptr(d_tc), len(src.table), 3, 1, _ptr(out), _ptr(fixes)) == _lib.E_NOMEM
        assert ctx.work_buffer_info()[1] == allocs0          # refused before the buffer was touched: nothing ran
        ctx.synchronize()
        assert (out == POISON).all() and (fixes == -0x5A5A5A5A5A5A5A5B).all()
        ctx.set_work_buffer_limit(need)                      # exactly the documented size: served (without a directory)
        assert fn(ctx._h, C.byref(r), k, _ptr(d_tk), _ptr(d_tc), len(src.table), 3, 1, _ptr(out), _ptr(fixes)) == _lib.OK
        expect, rows = correct_reads(host, n, L, k, dict_count(src.table), 3, 1)
        ctx.synchronize()
        assert (out.cpu().numpy() == expect).all() and (u64(fixes).reshape(n, 4) == rows).all()
    finally:
        ctx.set_work_buffer_limit(0)


# ---------------------------------------------------------------- robustness and determinism
@pytest.mark.parametrize("k", (31, 47))
def test_a_table_that_is_not_sorted(ctx, k):
    """random keys in random order with random counts: no expectation on the values -- the call returns, two calls give identical
    bytes, and nothing outside the output range changes"""
    import torch

    rng = np.random.default_rng(9900 + k)
    n, L = 300, 150
    host = random_reads(rng, n * L)
    host[rng.random(n * L) < 0.002] = ord("N")
    n_keys = 5000
    keys = rng.integers(0, 2**62, (n_keys, 2) if k > 31 else n_keys, dtype=np.uint64)
    if k > 31:
        keys[:, 1] &= np.uint64((1 << (2 * k - 64)) - 1)
    cnts = rng.integers(0, 2**63, n_keys, dtype=np.uint64)
    cnts[::3] = rng.integers(0, 4, len(cnts[::3]))
    d_tk, d_tc, bases = ctx.to_device(keys), ctx.to_device(cnts), ctx.to_device(host)
    runs = []
    for _ in range(2):
        whole = torch.full((GUARD + n * L + GUARD,), POISON, dtype=torch.uint8, device=ctx.device)
        out, rows = _fn(ctx, k)(bases, n, L, k, d_tk, d_tc, solid_min=2, min_cover=1, out=whole[GUARD:GUARD + n * L])
        ctx.synchronize()
        w = whole.cpu().numpy()
        assert (w[:GUARD] == POISON).all() and (w[-GUARD:] == POISON).all()
        runs.append((w.tobytes(), u64(rows).tobytes()))
    assert runs[0] == runs[1]
    assert (bases.cpu().numpy() == host).all()


@pytest.mark.parametrize("k", (15, 47))
def test_determinism(ctx, k):
    rng = np.random.default_rng(9950 + k)
    src = Source(rng, k)
    lens = _ragged_lens(rng, k, 300)
    n = len(lens)
    host = src.reads(rng, lens)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    src.add_weak(host, n, 0, offsets)
    d_tk, d_tc = _device_table(ctx, src.table, k)
    bases, d_off = ctx.to_device(host), ctx.to_device(offsets)
    a = _fn(ctx, k)(bases, n, 0, k, d_tk, d_tc, solid_min=3, min_cover=1, offsets=d_off)
    b = _fn(ctx, k)(bases, n, 0, k, d_tk, d_tc, solid_min=3, min_cover=1, offsets=d_off)
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and u64(a[1]).tobytes() == u64(b[1]).tobytes()
    assert int(u64(a[1])[:, 2].sum()) > 0 and (a[0] != bases).any()
