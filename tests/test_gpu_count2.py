"""Exact counting of two-word canonical k-mers, k = 33..64 (kmx_count_canonical2, kmx_count_merge2; kmx_count.hip) on the GPU.

The table is pinned to the multiset kmx_canonical_windows2 yields, as the oracle states it: canonical_windows2 -> valid windows ->
sorted as 2k-bit unsigned integers (high word first) -> run heads and lengths; bit-equal keys and counts, compared as uint64
(at k = 64 a quarter of the high words have their top bit set).  Case by case the shapes of test_gpu_count.py: every digit
alignment (2k mod 8 = 0, 2, 4, 6), uniform and ragged reads, odd base addresses, invalid bytes, FASTQ end to end, heavy hitters
and long shared prefixes (levels past the word boundary), keys that differ in one word only, layout edges, the contract.  At a size
the oracle cannot reach the table is checked against the composition of pinned calls on the device (kmx_canonical_windows2 ->
mask -> two stable sorts) and against kmx_canonical_reduce2's n_valid and word sums.  The read batches come from
tests/count_np.py."""
import ctypes as C

import numpy as np
import pytest

from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import dirty, random_reads, u64

pytestmark = pytest.mark.gpu

KS2 = (33, 34, 35, 40, 47, 48, 49, 56, 63, 64)


def _expect2(orc, host, n, L, k, offsets=None):
    _, _, canon, flags = orc.canonical_windows2(host, n, L, k, offsets=offsets)   # canon: (windows, 2) = (lo, hi)
    c = canon[(flags & 1) != 0]
    c = c[np.lexsort((c[:, 0], c[:, 1]))]                                         # hi first, then lo; uint64 compares unsigned
    head = np.ones(len(c), bool)
    head[1:] = (c[1:] != c[:-1]).any(axis=1)
    idx = np.nonzero(head)[0]
    return c[head], np.diff(np.append(idx, len(c))).astype(np.uint64)


def _check(ctx, orc, host, n, L, k, offsets=None, shift=0, expect=None):
    """host reads (uint8) -> count on the device at a base address `shift` bytes past an aligned one; bit-equal to the oracle"""
    buf = ctx.to_device(np.concatenate([np.zeros(shift, np.uint8), host, np.zeros(16, np.uint8)]))
    bases = buf[shift:shift + len(host)] if len(host) else buf[:0]
    d_off = None if offsets is None else ctx.to_device(np.asarray(offsets, np.uint64))
    km, cnt = ctx.count_canonical2(bases if len(host) else buf, n, L, k, offsets=d_off)
    ek, ec = expect if expect is not None else _expect2(orc, host, n, L, k, offsets)
    gk, gc = u64(km), u64(cnt)
    assert gk.shape == ek.shape, (k, L, n, shift, gk.shape, ek.shape)
    assert (gk == ek).all(), (k, L, n, shift)
    assert (gc == ec).all(), (k, L, n, shift)
    return gk, gc


def _check_shifts(ctx, orc, host, n, L, k, shifts, offsets=None):
    e = _expect2(orc, host, n, L, k, offsets)
    for s in shifts:
        out = _check(ctx, orc, host, n, L, k, offsets=offsets, shift=s, expect=e)
    return out


@pytest.mark.parametrize("k", KS2)
def test_uniform_reads(ctx, orc, k):
    rng = np.random.default_rng(1100 + k)
    for L, n in ((k, 5000), (150, 3000), (300, 700), (1000, 200)):
        host = random_reads(rng, n * L)
        _check_shifts(ctx, orc, host, n, L, k, (0, 1))   # aligned and odd d_bases


@pytest.mark.parametrize("k", KS2)
def test_invalid_bytes_and_lower_case(ctx, orc, k):
    rng = np.random.default_rng(1200 + k)
    for L, n in ((150, 4000), (300, 600)):
        host = random_reads(rng, n * L)
        for share in (0.005, 0.10):
            _check(ctx, orc, dirty(host, rng, share, n, L), n, L, k)
        h = dirty(host, rng, 0.10, n, L)
        h[7 * L:8 * L] = ord("N")                              # a read that is all N
        low = rng.random(n * L) < 0.3
        h[low & (h != ord("N")) & (h != ord(">"))] |= 0x20     # lower-case bases
        _check_shifts(ctx, orc, h, n, L, k, (0, 3))


@pytest.mark.parametrize("k", KS2)
@pytest.mark.parametrize("bound", (0, 160, 256, 1000))
def test_ragged_reads(ctx, orc, k, bound):
    rng = np.random.default_rng(1300 + k + bound)
    hi = {0: 200, 160: 160, 256: 256, 1000: 1000}[bound]
    n = 1500 if hi <= 256 else 300
    lens = rng.integers(0, hi + 1, n)
    lens[::17] = 0                             # empty reads
    lens[5::13] = k - 1                        # reads one base short of a window
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    host = random_reads(rng, int(offsets[-1]))
    bad = rng.random(len(host)) < 0.002
    host[bad] = ord("N")
    _check_shifts(ctx, orc, host, n, bound, k, (0, 5), offsets=offsets)   # (5: misaligned d_bases, the per-read kernels)


@pytest.mark.parametrize("k", (33, 47, 63))
def test_fastq_end_to_end(ctx, orc, k):
    from fastx_cases import fastq_text

    rng = np.random.default_rng(1400 + k)
    for text in (fastq_text(rng, 800, 0, 300), fastq_text(rng, 500, fixed=150)):
        bases, offsets = ctx.fastx_parse(ctx.to_device(text))
        n = int(offsets.numel()) - 1
        km, cnt = ctx.count_canonical2(bases, n, 300, k, offsets=offsets)
        eb, eo = orc.fastx_parse(text)
        ek, ec = _expect2(orc, np.asarray(eb, np.uint8), n, 300, k, np.asarray(eo, np.uint64))
        assert u64(km).shape == ek.shape
        assert (u64(km) == ek).all() and (u64(cnt) == ec).all()


@pytest.mark.parametrize("base", (b"A", b"T"))
def test_one_base_is_one_kmer(ctx, orc, base):
    """all A -> the key (0, 0), n (L - k + 1) times; all T likewise (its canonical form is all A)"""
    n, L = 20000, 150
    host = np.full(n * L, base[0], np.uint8)
    for k in (33, 48, 64):
        gk, gc = _check(ctx, orc, host, n, L, k)
        assert gk.tolist() == [[0, 0]] and gc.tolist() == [n * (L - k + 1)]


def test_heavy_hitter_and_shared_top_digits(ctx, orc):
    rng = np.random.default_rng(15)
    n, L = 20000, 150
    host = random_reads(rng, n * L)
    poly = rng.random(n) < 0.9                 # one k-mer ~90 % of the windows
    host.reshape(n, L)[poly] = ord("A")
    for k in (33, 47, 63):
        _check(ctx, orc, host, n, L, k)
    # poly-A with sparse substitutions: many distinct keys that share ALL their top digits (a substitution near the window's
    # start leaves the whole high word zero) -> partitions that stay large through the levels past the word boundary
    h = np.full(n * L, ord("A"), np.uint8)
    sub = rng.random(n * L) < 0.01
    h[sub] = random_reads(rng, int(sub.sum()))
    for k in (33, 47, 63):
        _check(ctx, orc, h, n, L, k)


def _reads_of(codes):
    """(m, k) base codes -> m reads of k bases as ASCII; base i of a read is bits [2i, 2i + 1] of its 2k-bit word (kmx.h)"""
    return np.frombuffer(b"ACGT", np.uint8)[codes].reshape(-1)


@pytest.mark.parametrize("k", (35, 47, 64))
def test_keys_that_differ_in_one_word_only(ctx, orc, k):
    """reads of k bases, one window each.  Bases 0..3 are A: the reverse complement then ends in TTTT at the top of the word, so
    the word itself is the canonical one unless its own top is TTTT too (the top base is kept A)."""
    rng = np.random.default_rng(1600 + k)
    m = 3000
    for vary_low in (True, False):
        codes = np.broadcast_to(rng.integers(0, 4, (1, k), dtype=np.uint8), (m, k)).copy()
        if vary_low:
            codes[:, 4:32] = rng.integers(0, 4, (m, 28), dtype=np.uint8)           # bases 0..31: the low word
        else:
            codes[:, 32:k] = rng.integers(0, 4, (m, k - 32), dtype=np.uint8)        # bases 32..k-1: the high word
        codes[:, :4] = 0
        codes[:, k - 1] = 0                     # (k = 35: two bases of the high word are left to vary, 16 keys)
        host = _reads_of(codes)
        gk, gc = _check(ctx, orc, host, m, k, k)
        fixed, moving = (1, 0) if vary_low else (0, 1)
        assert (gk[:, fixed] == gk[0, fixed]).all() and len(np.unique(gk[:, moving])) == len(gk)
        assert int(gc.sum()) == m
        g3, c3 = _check(ctx, orc, np.tile(host, 3), 3 * m, k, k)                    # each key three times as often
        assert (g3 == gk).all() and (c3 == 3 * gc).all()


def test_many_large_leaf_groups(ctx, orc):
    """Every top digit a partition of 513..4096 keys: level 0 leaves 256 groups on the large network"""
    rng = np.random.default_rng(112)
    k = 63
    # bases 0..3 A (see above), bases 59..62 the top digit, the 55 between random: 600 distinct 63-mers under each top digit
    codes = rng.integers(0, 4, (256, 600, k), dtype=np.uint8)
    codes[:, :, :4] = 0
    d = np.arange(256)
    for j in range(4):
        codes[:, :, 59 + j] = ((d >> (2 * j)) & 3)[:, None]
    host = _reads_of(codes.reshape(-1, k))
    m = 256 * 600
    ek, ec = _expect2(orc, host, m, k, k)
    top = (ek[:, 1] >> np.uint64(2 * k - 64 - 8)).astype(np.int64)
    assert len(ek) == m and (np.bincount(top, minlength=256) == 600).all() and (ec == 1).all()
    _check(ctx, orc, host, m, k, k, expect=(ek, ec))
    _check(ctx, orc, np.tile(host, 3), 3 * m, k, k, expect=(ek, 3 * ec))   # each key three times: partitions of 1800 keys


def test_even_k_palindromes(ctx, orc):
    n = 3000
    host = np.frombuffer(b"ACGT" * (n * 40), np.uint8)[: n * 150].copy()   # ACGT, GTAC, AATT ... are their own reverse complement
    host[150 * 10:150 * 20] = np.frombuffer(b"AATT" * 375, np.uint8)
    for k in (34, 40, 64):
        _check(ctx, orc, host, n, 150, k)


def test_big_random_batch_needs_every_level(ctx, orc):
    rng = np.random.default_rng(16)
    n, L = 40000, 150                           # ~4e6 windows: level-0 partitions of ~16k keys, then leaves
    host = random_reads(rng, n * L)
    for k in (33, 63):
        _check(ctx, orc, host, n, L, k)


def test_deep_coverage_of_a_small_genome(ctx, orc):
    """1.5e5 reads of 150 bases from a 30 kb genome (~600x): children of one k-mer with hundreds of copies, many of them"""
    rng = np.random.default_rng(113)
    g = random_reads(rng, 30_000)
    n, L = 150_000, 150
    starts = rng.integers(0, len(g) - L + 1, n)
    host = g[starts[:, None] + np.arange(L)[None, :]].reshape(-1).copy()
    rev = rng.random(n) < 0.5                                 # both strands
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    h2 = host.reshape(n, L)
    h2[rev] = comp[h2[rev][:, ::-1]]
    for k in (41, 63):
        _check(ctx, orc, host, n, L, k)


def test_no_window(ctx, orc):
    bases = ctx.to_device(np.full(8000, ord("A"), np.uint8))
    km, cnt = ctx.count_canonical2(bases, 100, 40, 47)            # reads shorter than k
    assert tuple(km.shape) == (0, 2) and cnt.numel() == 0
    nbuf = ctx.to_device(np.full(8000, ord("N"), np.uint8))
    km, cnt = ctx.count_canonical2(nbuf, 100, 80, 33)             # all N
    assert km.numel() == 0 and cnt.numel() == 0
    off = ctx.to_device(np.array([0, 0, 5, 10, 10], np.uint64))   # empty and short ragged reads
    km, _ = ctx.count_canonical2(bases, 4, 0, 63, offsets=off)
    assert km.numel() == 0


def _raw_count(ctx, bases, n, L, k, out_k, out_c, max_distinct):
    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    nd = C.c_uint64(12345)
    r = _lib.Reads(_ptr(bases), n, L, None)
    st = ctx.lib.kmx_count_canonical2(ctx._h, C.byref(r), k, _ptr(out_k), _ptr(out_c), max_distinct, C.byref(nd))
    return st, nd.value


def test_contract(ctx, orc):
    import torch

    from kmers_amd import _lib

    rng = np.random.default_rng(17)
    n, L, k = 3000, 150, 47
    host = random_reads(rng, n * L)
    host[rng.random(n * L) < 0.001] = ord("N")
    bases = ctx.to_device(host)
    ek, ec = _expect2(orc, host, n, L, k)
    nd = len(ek)
    sentinel = -0x5A5A5A5A5A5A5A5B
    ok_ = torch.full((2 * (nd + 8),), sentinel, dtype=torch.int64, device=ctx.device)
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
    st, _ = _raw_count(ctx, bases, n, L, k, None, oc, nd)
    assert st == _lib.E_ARG
    st, _ = _raw_count(ctx, bases, n, L, 32, ok_, oc, nd)
    assert st == _lib.E_K_RANGE
    st, _ = _raw_count(ctx, bases, n, L, 65, ok_, oc, nd)
    assert st == _lib.E_K_RANGE
    st, _ = _raw_count(ctx, bases, n, L, 31, ok_, oc, nd)     # (the one-word range belongs to kmx_count_canonical)
    assert st == _lib.E_K_RANGE
    assert (ok_ == sentinel).all() and (oc == sentinel).all()
    # a key array that is not 16-byte aligned: an argument error (keys move as 16-byte elements)
    st, _ = _raw_count(ctx, bases, n, L, k, ok_[1:], oc, nd)
    assert st == _lib.E_ARG
    # exactly the answer: written, and the slots behind it untouched
    st, got = _raw_count(ctx, bases, n, L, k, ok_, oc, nd)
    assert st == _lib.OK and got == nd
    assert (u64(ok_[:2 * nd]).reshape(-1, 2) == ek).all() and (u64(oc[:nd]) == ec).all()
    assert (ok_[2 * nd:] == sentinel).all() and (oc[nd:] == sentinel).all()
    # two calls, identical tables
    a = [u64(t) for t in ctx.count_canonical2(bases, n, L, k)]
    b = [u64(t) for t in ctx.count_canonical2(bases, n, L, k)]
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


def test_work_buffer_cap(ctx, orc):
    import torch

    from kmers_amd import _lib

    rng = np.random.default_rng(18)
    n, L, k = 4000, 150, 47
    host = random_reads(rng, n * L)
    bases = ctx.to_device(host)
    n_win = n * (L - k + 1)
    ok_ = torch.full((2 * n_win,), -1, dtype=torch.int64, device=ctx.device)
    oc = torch.full((n_win,), -1, dtype=torch.int64, device=ctx.device)
    try:
        # a cap far below the working set: refused before any kernel runs
        ctx.set_work_buffer_limit(1 << 20)
        allocs0 = ctx.work_buffer_info()[1]
        st, got = _raw_count(ctx, bases, n, L, k, ok_, oc, n_win)
        assert st == _lib.E_NOMEM
        assert ctx.work_buffer_info()[1] == allocs0          # refused before the buffer was touched: nothing ran
        assert (ok_ == -1).all() and (oc == -1).all()
        # the documented bound (kmx.h: at most 36 bytes per window + 1 MiB): a batch just inside it is served
        ctx.set_work_buffer_limit(36 * n_win + (1 << 20))
        st, got = _raw_count(ctx, bases, n, L, k, ok_, oc, n_win)
        assert st == _lib.OK
        ek, ec = _expect2(orc, host, n, L, k)
        assert got == len(ek) and (u64(ok_[:2 * got]).reshape(-1, 2) == ek).all() and (u64(oc[:got]) == ec).all()
    finally:
        ctx.set_work_buffer_limit(0)


def _merge_check(ctx, orc, ha, hb, n, L, k):
    ka, ca = ctx.count_canonical2(ctx.to_device(ha), n, L, k) if len(ha) else ctx.count_canonical2(ctx.to_device(hb), 0, L, k)
    kb, cb = ctx.count_canonical2(ctx.to_device(hb), n, L, k) if len(hb) else ctx.count_canonical2(ctx.to_device(ha), 0, L, k)
    mk, mc = ctx.count_merge2(ka, ca, kb, cb)
    both = np.concatenate([ha, hb])
    ek, ec = _expect2(orc, both, len(both) // L, L, k)
    assert u64(mk).shape == ek.shape
    assert (u64(mk) == ek).all() and (u64(mc) == ec).all()
    return mk, mc, ka, ca, kb, cb


@pytest.mark.parametrize("k", (33, 47, 64))
def test_merge(ctx, orc, k):
    from kmers_amd import _lib

    rng = np.random.default_rng(1900 + k)
    n, L = 3000, 150
    a = random_reads(rng, n * L)
    b = random_reads(rng, n * L)
    _merge_check(ctx, orc, a, b, n, L, k)                                  # disjoint
    _merge_check(ctx, orc, a, a.copy(), n, L, k)                           # identical
    _merge_check(ctx, orc, a, np.zeros(0, np.uint8), n, L, k)              # one empty
    _merge_check(ctx, orc, np.zeros(0, np.uint8), b, n, L, k)
    over = np.concatenate([a[: n * L // 2], b[: n * L // 2]])              # overlapping
    mk, mc, ka, ca, kb, cb = _merge_check(ctx, orc, a, over, n, L, k)
    with pytest.raises(_lib.KmxError) as ei:
        ctx.count_merge2(ka, ca, kb, cb, max_out=int(mc.numel()) - 1)
    assert ei.value.status == _lib.E_NOMEM


@pytest.mark.parametrize("k", (47, 63))
@pytest.mark.parametrize("dirty", (False, True))
def test_at_size(ctx, k, dirty):
    """5e6 reads of 150 bases (5.2e8 windows at k = 47: ~19 GB of working set at 36 bytes per window, inside the automatic cap of
    a 288 GB device): the pinned summary, and the composition of pinned calls"""
    import torch

    n, L = 5_000_000, 150
    bases = ctx.gen_reads(n * L, seed=0xC0FFEE + k)
    if dirty:
        g = torch.Generator(device=ctx.device).manual_seed(k)
        rows = torch.nonzero(torch.rand(n, device=ctx.device, generator=g) < 0.02).flatten()
        pos = torch.randint(0, L, (rows.numel(),), device=ctx.device, generator=g)
        bases[rows * L + pos] = ord("N")
    km, cnt = ctx.count_canonical2(bases, n, L, k)
    s = ctx.canonical_reduce2(bases, n, L, k)
    assert int(cnt.sum().item()) == s.n_valid
    # kmx_summary2.sum_lo / sum_hi are the wrapping sums of the canonical words' low / high words, each on its own (sum_lo is
    # also the low half of the 128-bit sum): sum of word * count mod 2^64 (int64 arithmetic wraps like u64)
    assert int((km[:, 0] * cnt).sum().item()) & (2**64 - 1) == s.sum_lo
    assert int((km[:, 1] * cnt).sum().item()) & (2**64 - 1) == s.sum_hi
    # the composition: kmx_canonical_windows2 -> mask -> both words XOR 1 << 63 (signed order = unsigned order) -> stable sort by
    # the low word, then stable by the high word -> run heads and lengths
    w = ctx.canonical_windows2(bases, n, L, k)
    del w["fw"], w["rc"]
    valid = (w["flags"] & 1) != 0
    canon = w["canon"].view(-1, 2)
    # (each word masked, sorted and gathered as a dense 1-D array of its own: a row gather of the (N, 2) tensor by 1e8 and more
    # indices came back wrong from torch 2.10 on ROCm 7.0, 2^26 rows of it, while 1-D gathers of 5e8 are right)
    lo = canon[:, 0][valid] ^ torch.iinfo(torch.int64).min
    hi = canon[:, 1][valid] ^ torch.iinfo(torch.int64).min
    del w, canon, valid
    p = torch.sort(lo, stable=True).indices
    lo, hi = lo[p], hi[p]
    p = torch.sort(hi, stable=True).indices
    lo, hi = lo[p], hi[p]
    del p
    head = torch.ones(lo.numel(), dtype=torch.bool, device=lo.device)
    head[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    idx = torch.nonzero(head).flatten()
    uk = torch.stack((lo[idx], hi[idx]), dim=1) ^ torch.iinfo(torch.int64).min
    uc = torch.diff(idx, append=torch.tensor([lo.numel()], device=lo.device))
    del lo, hi, head, idx
    assert tuple(uk.shape) == tuple(km.shape)
    assert torch.equal(uk, km) and torch.equal(uc, cnt)
