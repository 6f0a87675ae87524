"""Exact canonical k-mer counting (kmx_count_canonical, kmx_count_merge; kmx_count.hip) on the GPU.

The table is pinned to the multiset CanonicalKmerIterator yields (canonical_kmer_iterator.rs:42-116): the oracle's windows,
np.unique(canon[flags & 1], return_counts=True), bit-equal keys and counts -- for every k-mer width, uniform and ragged
reads, odd base addresses, invalid bytes, FASTQ end to end, heavy hitters and layout edges.  At a size the oracle cannot
reach, the table is checked against the composition of already-pinned calls (kmx_canonical_windows -> mask -> torch.unique)
and against kmx_canonical_reduce's n_valid / sum_canon.  The read batches come from tests/count_np.py."""
import ctypes as C

import numpy as np
import pytest

from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import dirty, random_reads, u64

pytestmark = pytest.mark.gpu

KS = (1, 2, 5, 9, 12, 13, 21, 31)


def _expect(orc, host, n, L, k, offsets=None):
    _, _, canon, flags = orc.canonical_windows(host, n, L, k, offsets=offsets)
    return np.unique(canon[(flags & 1) != 0], return_counts=True)


def _check(ctx, orc, host, n, L, k, offsets=None, shift=0):
    """host reads (uint8) -> count on the device at a base address `shift` bytes past an aligned one; bit-equal to the oracle"""
    buf = ctx.to_device(np.concatenate([np.zeros(shift, np.uint8), host, np.zeros(16, np.uint8)]))
    bases = buf[shift:shift + len(host)] if len(host) else buf[:0]
    d_off = None if offsets is None else ctx.to_device(np.asarray(offsets, np.uint64))
    km, cnt = ctx.count_canonical(bases if len(host) else buf, n, L, k, offsets=d_off)
    ek, ec = _expect(orc, host, n, L, k, offsets)
    gk, gc = u64(km), u64(cnt)
    assert gk.shape == ek.shape, (k, L, n, shift, gk.shape, ek.shape)
    assert (gk == ek).all(), (k, L, n, shift)
    assert (gc == ec.astype(np.uint64)).all(), (k, L, n, shift)
    return gk, gc


@pytest.mark.parametrize("k", KS)
def test_uniform_reads(ctx, orc, k):
    rng = np.random.default_rng(100 + k)
    for L, n in ((k, 5000), (150, 3000), (300, 700), (1000, 200)):
        host = random_reads(rng, n * L)
        _check(ctx, orc, host, n, L, k)
        _check(ctx, orc, host, n, L, k, shift=1)   # odd d_bases


@pytest.mark.parametrize("k", KS)
def test_invalid_bytes_and_lower_case(ctx, orc, k):
    rng = np.random.default_rng(200 + k)
    for L, n in ((150, 4000), (300, 600)):
        host = random_reads(rng, n * L)
        for share in (0.005, 0.10):
            _check(ctx, orc, dirty(host, rng, share, n, L), n, L, k)
        h = dirty(host, rng, 0.10, n, L)
        h[7 * L:8 * L] = ord("N")                              # a read that is all N
        low = rng.random(n * L) < 0.3
        h[low & (h != ord("N")) & (h != ord(">"))] |= 0x20     # lower-case bases
        _check(ctx, orc, h, n, L, k)
        _check(ctx, orc, h, n, L, k, shift=3)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("bound", (0, 160, 256, 1000))
def test_ragged_reads(ctx, orc, k, bound):
    rng = np.random.default_rng(300 + k + bound)
    hi = {0: 200, 160: 160, 256: 256, 1000: 1000}[bound]
    n = 1500 if hi <= 256 else 300
    lens = rng.integers(0, hi + 1, n)
    lens[::17] = 0                             # empty reads
    lens[5::13] = max(k - 1, 0)                # reads shorter than k
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    host = random_reads(rng, int(offsets[-1]))
    bad = rng.random(len(host)) < 0.002
    host[bad] = ord("N")
    _check(ctx, orc, host, n, bound, k, offsets=offsets)
    _check(ctx, orc, host, n, bound, k, offsets=offsets, shift=5)   # misaligned d_bases: the per-read kernels


@pytest.mark.parametrize("k", (5, 13, 31))
def test_fastq_end_to_end(ctx, orc, k):
    from fastx_cases import fastq_text

    rng = np.random.default_rng(400 + k)
    for text in (fastq_text(rng, 800, 0, 300), fastq_text(rng, 500, fixed=150)):
        bases, offsets = ctx.fastx_parse(ctx.to_device(text))
        n = int(offsets.numel()) - 1
        km, cnt = ctx.count_canonical(bases, n, 300, k, offsets=offsets)
        eb, eo = orc.fastx_parse(text)
        ek, ec = _expect(orc, np.asarray(eb, np.uint8), n, 300, k, np.asarray(eo, np.uint64))
        assert (u64(km) == ek).all() and (u64(cnt) == ec.astype(np.uint64)).all()


def test_all_a_is_one_kmer(ctx, orc):
    n, L = 20000, 150
    host = np.full(n * L, ord("A"), np.uint8)
    for k in (1, 12, 31):
        gk, gc = _check(ctx, orc, host, n, L, k)
        assert list(gk) == [0] and list(gc) == [n * (L - k + 1)]


def test_heavy_hitter_and_shared_top_digits(ctx, orc):
    rng = np.random.default_rng(5)
    n, L = 20000, 150
    host = random_reads(rng, n * L)
    poly = rng.random(n) < 0.9                 # one k-mer ~90 % of the windows
    host.reshape(n, L)[poly] = ord("A")
    for k in (9, 21, 31):
        _check(ctx, orc, host, n, L, k)
    # poly-A with sparse substitutions: many distinct keys that share their top digits -> partitions far above a block's LDS
    h = np.full(n * L, ord("A"), np.uint8)
    sub = rng.random(n * L) < 0.01
    h[sub] = random_reads(rng, int(sub.sum()))
    for k in (13, 21, 31):
        _check(ctx, orc, h, n, L, k)


def test_even_k_palindromes(ctx, orc):
    n = 3000
    host = np.frombuffer(b"ACGT" * (n * 40), np.uint8)[: n * 150].copy()   # ACGT, GTAC, AATT ... are their own reverse complement
    host[150 * 10:150 * 20] = np.frombuffer(b"AATT" * 375, np.uint8)
    for k in (2, 4, 6, 10):
        _check(ctx, orc, host, n, 150, k)


def test_big_random_batch_needs_every_level(ctx, orc):
    rng = np.random.default_rng(6)
    n, L = 40000, 150                           # 4.8e6 windows: level-0 partitions of ~19k keys, then leaves
    host = random_reads(rng, n * L)
    for k in (12, 31):
        _check(ctx, orc, host, n, L, k)


def _decode(keys, k):
    """u64 k-mer words -> their bases as ASCII, base i at bits [2i, 2i + 1] (kmx.h)"""
    codes = (keys[:, None] >> (2 * np.arange(k, dtype=np.uint64))[None, :]) & np.uint64(3)
    return np.frombuffer(b"ACGT", np.uint8)[codes.astype(np.int64)]


def _canonical(codes):
    k = codes.shape[1]
    sh = (2 * np.arange(k, dtype=np.uint64))[None, :]
    fw = (codes.astype(np.uint64) << sh).sum(axis=1, dtype=np.uint64)
    rc = ((3 - codes[:, ::-1]).astype(np.uint64) << sh).sum(axis=1, dtype=np.uint64)
    return np.minimum(fw, rc)


def test_many_large_leaf_groups(ctx, orc):
    """Every top digit a partition of 513..4096 keys: level 0 leaves 256 groups on the large network (their bound once fell short)"""
    rng = np.random.default_rng(12)
    k = 31
    # bases 0..3 A (the reverse complement then starts with TTTT, so the word itself is canonical and keeps its top digit), bases
    # 27..30 the top digit, the 23 between random: 600 distinct canonical 31-mers under each of the 256 top digits
    codes = rng.integers(0, 4, (256, 700, k), dtype=np.uint8)
    codes[:, :, :4] = 0
    d = np.arange(256)
    for j in range(4):
        codes[:, :, 27 + j] = ((d >> (2 * j)) & 3)[:, None]
    keys = [np.unique(_canonical(codes[i]))[:600] for i in range(256)]
    assert all(len(x) == 600 and ((x >> np.uint64(2 * k - 8)) == i).all() for i, x in enumerate(keys))
    pick = np.concatenate(keys)
    host = _decode(pick, k).reshape(-1)
    gk, gc = _check(ctx, orc, host, len(pick), k, k)       # reads of k bases: one window, one key each
    assert len(gk) == len(pick) and (gc == 1).all()
    gk, gc = _check(ctx, orc, np.tile(host, 3), 3 * len(pick), k, k)   # each key three times: partitions of 1800 keys
    assert (gc == 3).all()


def test_deep_coverage_of_a_small_genome(ctx, orc):
    """1.5e5 reads of 150 bases from a 30 kb genome (~600x): children of one k-mer with hundreds of copies, many of them"""
    rng = np.random.default_rng(13)
    g = random_reads(rng, 30_000)
    n, L = 150_000, 150
    starts = rng.integers(0, len(g) - L + 1, n)
    host = g[starts[:, None] + np.arange(L)[None, :]].reshape(-1).copy()
    rev = rng.random(n) < 0.5                                 # both strands
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    h2 = host.reshape(n, L)
    h2[rev] = comp[h2[rev][:, ::-1]]
    for k in (21, 31):
        _check(ctx, orc, host, n, L, k)


def test_no_window(ctx, orc):
    bases = ctx.to_device(np.full(4000, ord("A"), np.uint8))
    km, cnt = ctx.count_canonical(bases, 100, 20, 31)
    assert km.numel() == 0 and cnt.numel() == 0
    nbuf = ctx.to_device(np.full(4000, ord("N"), np.uint8))
    km, _ = ctx.count_canonical(nbuf, 100, 40, 21)
    assert km.numel() == 0
    off = ctx.to_device(np.array([0, 0, 5, 10], np.uint64))
    km, _ = ctx.count_canonical(bases, 3, 0, 31, offsets=off)
    assert km.numel() == 0


def _raw_count(ctx, bases, n, L, k, out_k, out_c, max_distinct):
    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    nd = C.c_uint64(12345)
    r = _lib.Reads(_ptr(bases), n, L, None)
    st = ctx.lib.kmx_count_canonical(ctx._h, C.byref(r), k, _ptr(out_k), _ptr(out_c), max_distinct, C.byref(nd))
    return st, nd.value


def test_contract(ctx, orc):
    import torch

    from kmers_amd import _lib

    rng = np.random.default_rng(7)
    n, L, k = 3000, 150, 13
    host = random_reads(rng, n * L)
    host[rng.random(n * L) < 0.001] = ord("N")
    bases = ctx.to_device(host)
    ek, ec = _expect(orc, host, n, L, k)
    nd = len(ek)
    sentinel = -0x5A5A5A5A5A5A5A5B
    ok_ = torch.full((nd + 8,), sentinel, dtype=torch.int64, device=ctx.device)
    oc = torch.full((nd + 8,), sentinel, dtype=torch.int64, device=ctx.device)
    # one below the answer: KMX_E_NOMEM, the right count, outputs untouched
    st, got = _raw_count(ctx, bases, n, L, k, ok_, oc, nd - 1)
    assert st == _lib.E_NOMEM and got == nd
    assert (ok_ == sentinel).all() and (oc == sentinel).all()
    # NULL outputs: the count only
    st, got = _raw_count(ctx, bases, n, L, k, None, None, 0)
    assert st == _lib.OK and got == nd
    # one output NULL, the other not: an argument error before anything runs; k out of range likewise
    st, _ = _raw_count(ctx, bases, n, L, k, ok_, None, nd)
    assert st == _lib.E_ARG
    st, _ = _raw_count(ctx, bases, n, L, 32, ok_, oc, nd)
    assert st == _lib.E_K_RANGE
    st, _ = _raw_count(ctx, bases, n, L, 0, ok_, oc, nd)
    assert st == _lib.E_K_RANGE
    # exactly the answer: written, and the slots behind it untouched
    st, got = _raw_count(ctx, bases, n, L, k, ok_, oc, nd)
    assert st == _lib.OK and got == nd
    assert (u64(ok_[:nd]) == ek).all() and (u64(oc[:nd]) == ec.astype(np.uint64)).all()
    assert (ok_[nd:] == sentinel).all()
    # two calls, identical tables
    a = [u64(t) for t in ctx.count_canonical(bases, n, L, k)]
    b = [u64(t) for t in ctx.count_canonical(bases, n, L, k)]
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


def test_work_buffer_cap(ctx, orc):
    import torch

    from kmers_amd import _lib

    rng = np.random.default_rng(8)
    n, L, k = 4000, 150, 31
    host = random_reads(rng, n * L)
    bases = ctx.to_device(host)
    n_win = n * (L - k + 1)
    ok_ = torch.full((n_win,), -1, dtype=torch.int64, device=ctx.device)
    oc = torch.full((n_win,), -1, dtype=torch.int64, device=ctx.device)
    try:
        # a cap far below the working set: refused before any kernel runs
        ctx.set_work_buffer_limit(1 << 20)
        allocs0 = ctx.work_buffer_info()[1]
        st, got = _raw_count(ctx, bases, n, L, k, ok_, oc, n_win)
        assert st == _lib.E_NOMEM
        assert ctx.work_buffer_info()[1] == allocs0          # refused before the buffer was touched: nothing ran
        assert (ok_ == -1).all() and (oc == -1).all()
        # the documented bound (kmx.h: at most 20 bytes per window + 1 MiB): a batch just inside it is served
        ctx.set_work_buffer_limit(20 * n_win + (1 << 20))
        st, got = _raw_count(ctx, bases, n, L, k, ok_, oc, n_win)
        assert st == _lib.OK
        ek, ec = _expect(orc, host, n, L, k)
        assert got == len(ek) and (u64(ok_[:got]) == ek).all() and (u64(oc[:got]) == ec.astype(np.uint64)).all()
    finally:
        ctx.set_work_buffer_limit(0)


def _table(orc, host, n, L, k):
    ek, ec = _expect(orc, host, n, L, k)
    return ek, ec.astype(np.uint64)


def _merge_check(ctx, orc, ha, hb, n, L, k):
    ka, ca = ctx.count_canonical(ctx.to_device(ha), n, L, k) if len(ha) else ctx.count_canonical(ctx.to_device(hb), 0, L, k)
    kb, cb = ctx.count_canonical(ctx.to_device(hb), n, L, k) if len(hb) else ctx.count_canonical(ctx.to_device(ha), 0, L, k)
    mk, mc = ctx.count_merge(ka, ca, kb, cb)
    both = np.concatenate([ha, hb])
    ek, ec = _table(orc, both, len(both) // L, L, k)
    assert (u64(mk) == ek).all() and (u64(mc) == ec).all()
    return mk, mc, ka, ca, kb, cb


def test_merge(ctx, orc):
    from kmers_amd import _lib

    rng = np.random.default_rng(9)
    n, L, k = 3000, 150, 21
    a = random_reads(rng, n * L)
    b = random_reads(rng, n * L)
    _merge_check(ctx, orc, a, b, n, L, k)                                  # (almost surely) disjoint
    _merge_check(ctx, orc, a, a.copy(), n, L, k)                           # identical
    _merge_check(ctx, orc, a, np.zeros(0, np.uint8), n, L, k)              # one empty
    _merge_check(ctx, orc, np.zeros(0, np.uint8), b, n, L, k)
    over = np.concatenate([a[: n * L // 2], b[: n * L // 2]])              # overlapping
    mk, mc, ka, ca, kb, cb = _merge_check(ctx, orc, a, over, n, L, k)
    with pytest.raises(_lib.KmxError) as ei:
        ctx.count_merge(ka, ca, kb, cb, max_out=int(mk.numel()) - 1)
    assert ei.value.status == _lib.E_NOMEM
    # small k: nearly every key in both tables
    _merge_check(ctx, orc, a, b, n, L, 4)


@pytest.mark.parametrize("k", (31, 21))
@pytest.mark.parametrize("dirty", (False, True))
def test_at_size(ctx, k, dirty):
    """1e7 reads of 150 bases: the composition of pinned calls, and the pinned summary"""
    import torch

    from kmers_amd import _lib

    n, L = 10_000_000, 150
    bases = ctx.gen_reads(n * L, seed=0xC0FFEE + k)
    if dirty:
        g = torch.Generator(device=ctx.device).manual_seed(k)
        rows = torch.nonzero(torch.rand(n, device=ctx.device, generator=g) < 0.02).flatten()
        pos = torch.randint(0, L, (rows.numel(),), device=ctx.device, generator=g)
        bases[rows * L + pos] = ord("N")
    km, cnt = ctx.count_canonical(bases, n, L, k)
    s = ctx.canonical_reduce(bases, n, L, k, _lib.HASH_NONE, 0)
    assert int(cnt.sum().item()) == s.n_valid
    # sum of kmer * count mod 2^64 (int64 arithmetic wraps like u64)
    assert int((km * cnt).sum().item()) & (2**64 - 1) == s.sum_canon
    # the composition: kmx_canonical_windows -> mask -> torch.unique (keys < 2^62: the signed order is the unsigned one)
    w = ctx.canonical_windows(bases, n, L, k, want=("canon", "flags"))
    keys = w["canon"][(w["flags"] & 1) != 0]
    del w
    uk, uc = torch.unique(keys, sorted=True, return_counts=True)
    del keys
    assert uk.numel() == km.numel()
    assert torch.equal(uk, km) and torch.equal(uc, cnt)
