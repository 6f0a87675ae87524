"""Queries on a count table on the GPU: kmx_count_lookup(2), kmx_count_lookup_reads(2), kmx_count_spectrum, kmx_count_filter(2)
(kmx_count_query.hip).

Everything is exact (u64 equality).  The lookup is pinned to the oracle: table = np.unique of the oracle's valid canonical words of
batch A (thinned on the host), queries = the oracle's canonical words and flags of batch B, expected = np.searchsorted + equality on
the host (tests/count_np.py: table_of and host_lookup, numpy and not the code under test).  Every such test asserts of
its own input that at least a tenth of the valid queries hit and at least a tenth miss.  The reads form is pinned to the
composition canonical_windows(2) -> count_lookup(2) and to the oracle route; spectrum to np.bincount; filter to boolean indexing.
At a size the oracle cannot reach: the composition of pinned calls on the device (k = 31), a host search of 10^6 sampled windows
(k = 47), and the identity sum(d_out) == sum(count ** 2) of a batch looked up in its own table."""
import ctypes as C

import numpy as np
import pytest

from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import dirty, host_lookup, orc_windows, random_reads, table_of, two_batches, u64, words

pytestmark = pytest.mark.gpu

KS1 = (1, 2, 5, 9, 12, 13, 21, 31)
KS2 = (33, 34, 35, 47, 63, 64)
U64_MAX = 2**64 - 1


def _dev_lookup(ctx, tk, tc, k, q, qflags=None, out=None):
    f = ctx.count_lookup if k <= 31 else ctx.count_lookup2
    return u64(f(ctx.to_device(tk), None if tc is None else ctx.to_device(tc), k, q if not isinstance(q, np.ndarray) else ctx.to_device(q),
                 None if qflags is None else ctx.to_device(qflags), out=out))


def _thin(tk, tc):
    keep = np.arange(len(tk)) % 3 != 0           # every third entry dropped: still a table
    return tk[keep], tc[keep]


def _assert_hits_and_misses(expect, qflags):
    valid = (qflags & 1) != 0
    nv = int(valid.sum())
    hits = int((expect[valid] != 0).sum())
    assert nv > 0 and 10 * hits >= nv and 10 * (nv - hits) >= nv, (nv, hits)


# ---------------------------------------------------------------- lookup against the oracle
@pytest.mark.parametrize("k", KS1 + KS2)
def test_lookup_against_the_oracle(ctx, orc, k):
    rng = np.random.default_rng(2100 + k)
    n, L = 3000, 150
    a, b = two_batches(rng, n, L)
    tk, tc = _thin(*table_of(*orc_windows(orc, a, n, L, k)))
    q, qf = orc_windows(orc, b, n, L, k)
    expect = host_lookup(tk, tc, q, qf)
    _assert_hits_and_misses(expect, qf)
    got = _dev_lookup(ctx, tk, tc, k, q, qf)
    assert (got == expect).all(), k
    assert (_dev_lookup(ctx, tk, tc, k, q, None) == host_lookup(tk, tc, q, None)).all()      # no flags
    assert (_dev_lookup(ctx, tk, None, k, q, qf) == (expect != 0).astype(np.uint64)).all()    # membership
    # determinism: two calls, bit-identical
    assert (_dev_lookup(ctx, tk, tc, k, q, qf) == got).all()


@pytest.mark.parametrize("k", (5, 13, 31, 33, 47, 64))
def test_lookup_flags_of_a_dirty_batch(ctx, orc, k):
    rng = np.random.default_rng(2200 + k)
    n, L = 3000, 150
    a, b = two_batches(rng, n, L)
    b = dirty(b, rng, 0.2, n, L)
    tk, tc = _thin(*table_of(*orc_windows(orc, a, n, L, k)))
    q, qf = orc_windows(orc, b, n, L, k)
    bad = np.nonzero((qf & 1) == 0)[0]
    assert len(bad) > 1000
    q = q.copy()
    q[bad] = tk[rng.integers(0, len(tk), len(bad))]     # words that ARE in the table, in slots that are not valid
    expect = host_lookup(tk, tc, q, qf)
    assert (expect[bad] == 0).all() and (host_lookup(tk, tc, q, None)[bad] != 0).all()
    _assert_hits_and_misses(expect, qf)
    assert (_dev_lookup(ctx, tk, tc, k, q, qf) == expect).all()


@pytest.mark.parametrize("k", (9, 21, 31))
def test_lookup_in_place(ctx, orc, k):
    rng = np.random.default_rng(2300 + k)
    n, L = 3000, 150
    a, b = two_batches(rng, n, L)
    tk, tc = _thin(*table_of(*orc_windows(orc, a, n, L, k)))
    q, qf = orc_windows(orc, b, n, L, k)
    expect = host_lookup(tk, tc, q, qf)
    _assert_hits_and_misses(expect, qf)
    d_q = ctx.to_device(q)
    out = ctx.count_lookup(ctx.to_device(tk), ctx.to_device(tc), k, d_q, ctx.to_device(qf), out=d_q)
    assert out.data_ptr() == d_q.data_ptr()
    assert (u64(d_q) == expect).all()


def _synthetic_table(rng, k, n, lo_bits=None, prefixes=None):
    """n distinct sorted keys of 2k bits: all bits random, or only the low `lo_bits` (every key in ONE directory bin), or a few
    values of the top 24 bits (most bins empty)"""
    w = words(k)
    bits = 2 * k
    vals = set()
    while len(vals) < n:
        m = n - len(vals) + 16
        v = [int.from_bytes(rng.bytes(16), "little") & ((1 << (lo_bits or bits)) - 1) for _ in range(m)]
        if prefixes is not None:
            v = [(x & ((1 << (bits - 24)) - 1)) | (int(prefixes[i % len(prefixes)]) << (bits - 24)) for i, x in enumerate(v)]
        vals.update(v)
    vals = sorted(vals)[:n]
    if w == 1:
        tk = np.array(vals, np.uint64)
    else:
        tk = np.array([[v & U64_MAX, v >> 64] for v in vals], np.uint64)
    tc = rng.integers(1, 1000, n).astype(np.uint64)
    return tk, tc


def _queries_from(rng, tk, m):
    """half present keys, half keys nudged by one (mostly absent)"""
    q = tk[rng.integers(0, len(tk), m)].copy()
    odd = np.arange(m) % 2 == 1
    if q.ndim == 1:
        q[odd] ^= np.uint64(1)
    else:
        q[odd, 0] ^= np.uint64(1)
    return q


@pytest.mark.parametrize("k", (31, 35, 64))
@pytest.mark.parametrize("shape", ("one_bin", "sparse_bins", "spread"))
def test_lookup_skewed_tables(ctx, k, shape):
    rng = np.random.default_rng(2400 + k + len(shape))
    n = 50000
    if shape == "one_bin":
        tk, tc = _synthetic_table(rng, k, n, lo_bits=30)           # the top 2k - 30 bits all zero
    elif shape == "sparse_bins":
        tk, tc = _synthetic_table(rng, k, n, prefixes=(1, 2, 3, 0x7FFFF, 0xFFFFF))
    else:
        tk, tc = _synthetic_table(rng, k, n)
    q = _queries_from(rng, tk, 200000)                             # enough queries for the directory
    expect = host_lookup(tk, tc, q)
    assert 10 * int((expect != 0).sum()) >= len(q) and 10 * int((expect == 0).sum()) >= len(q)
    assert (_dev_lookup(ctx, tk, tc, k, q) == expect).all()
    # the same with a batch small enough for the plain search, and with no room for a directory: same answers, no KMX_E_NOMEM
    small = q[:300]
    assert (_dev_lookup(ctx, tk, tc, k, small) == expect[:300]).all()
    try:
        ctx.set_work_buffer_limit(4096)
        assert (_dev_lookup(ctx, tk, tc, k, q) == expect).all()
    finally:
        ctx.set_work_buffer_limit(0)


@pytest.mark.parametrize("k", (1, 13, 31, 33, 47, 64))
def test_lookup_edges(ctx, k):
    import torch

    rng = np.random.default_rng(2500 + k)
    w = words(k)
    n = min(3000, 4 ** k // 2)
    tk, tc = _synthetic_table(rng, k, n)
    shape = (0,) if w == 1 else (0, 2)
    d_tk, d_tc = ctx.to_device(tk), ctx.to_device(tc)
    f = ctx.count_lookup if w == 1 else ctx.count_lookup2
    # n = 0: every answer 0 (the output is overwritten); n_query = 0: a no-op
    q = _queries_from(rng, tk, 5000)
    out = torch.full((len(q),), -1, dtype=torch.int64, device=ctx.device)
    f(ctx.to_device(np.zeros(shape, np.uint64)), d_tc[:0], k, ctx.to_device(q), out=out)
    assert (out == 0).all()
    assert f(d_tk, d_tc, k, ctx.to_device(np.zeros(shape, np.uint64))).numel() == 0
    def as_q(vals):
        return np.array(vals, np.uint64) if w == 1 else np.array([[v & U64_MAX, v >> 64] for v in vals], np.uint64)

    def as_int(row):
        return int(row) if w == 1 else int(row[0]) | (int(row[1]) << 64)

    first, last = as_int(tk[0]), as_int(tk[-1])
    assert first < last
    # n = 1
    one = _dev_lookup(ctx, tk[:1], tc[:1], k, as_q([first, last, first]))
    assert one.tolist() == [int(tc[0]), 0, int(tc[0])]
    # the smallest and the largest key; below the first and above the last; a bit at or above 2k
    vals = [first, last]
    expect = [int(tc[0]), int(tc[-1])]
    if first > 0:
        vals.append(first - 1)
        expect.append(0)
    if last + 1 < 4 ** k:
        vals.append(last + 1)
        expect.append(0)
    if k not in (64,):
        vals += [first | (1 << (2 * k)), last | (1 << (2 * k)), first | (1 << (64 * w - 1))]   # (k = 64: there is no such bit)
        expect += [0, 0, 0]
    for m in (len(vals), 4096):                          # alone (plain search) and among enough queries for the directory
        qv = as_q(vals + [first] * (m - len(vals)))
        got = _dev_lookup(ctx, tk, tc, k, qv)
        assert got[:len(vals)].tolist() == expect and (got[len(vals):] == tc[0]).all(), (k, m)
    # one query repeated 10^6 times
    rep = as_q([last] * 1_000_000)
    assert (_dev_lookup(ctx, tk, tc, k, rep) == tc[-1]).all()


def test_lookup_all_a_table(ctx, orc):
    n, L = 2000, 150
    host = np.full(n * L, ord("A"), np.uint8)
    for k in (31, 47):
        tk, tc = table_of(*orc_windows(orc, host, n, L, k))
        assert len(tk) == 1 and int(tc[0]) == n * (L - k + 1)
        rng = np.random.default_rng(k)
        b = random_reads(rng, n * L)
        b.reshape(n, L)[::2] = ord("T")                  # poly-T: canonical form all A
        q, qf = orc_windows(orc, b, n, L, k)
        expect = host_lookup(tk, tc, q, qf)
        _assert_hits_and_misses(expect, qf)
        assert (_dev_lookup(ctx, tk, tc, k, q, qf) == expect).all()


def test_lookup_contract(ctx):
    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    rng = np.random.default_rng(26)
    tk, tc = _synthetic_table(rng, 47, 1000)
    d_tk, d_tc = ctx.to_device(tk).view(-1), ctx.to_device(tc)
    q = ctx.to_device(tk[:10]).view(-1)
    out = ctx.empty(16, __import__("torch").int64)
    lib, h = ctx.lib, ctx._h
    assert lib.kmx_count_lookup2(h, _ptr(d_tk), _ptr(d_tc), 1000, 32, _ptr(q), None, 10, _ptr(out)) == _lib.E_K_RANGE
    assert lib.kmx_count_lookup2(h, _ptr(d_tk), _ptr(d_tc), 1000, 65, _ptr(q), None, 10, _ptr(out)) == _lib.E_K_RANGE
    assert lib.kmx_count_lookup(h, _ptr(d_tk), _ptr(d_tc), 1000, 32, _ptr(q), None, 10, _ptr(out)) == _lib.E_K_RANGE
    assert lib.kmx_count_lookup(h, _ptr(d_tk), _ptr(d_tc), 1000, 0, _ptr(q), None, 10, _ptr(out)) == _lib.E_K_RANGE
    assert lib.kmx_count_lookup2(h, _ptr(d_tk[1:]), _ptr(d_tc), 999, 47, _ptr(q), None, 10, _ptr(out)) == _lib.E_ARG      # misaligned keys
    assert lib.kmx_count_lookup2(h, _ptr(d_tk), _ptr(d_tc), 1000, 47, _ptr(q[1:]), None, 9, _ptr(out)) == _lib.E_ARG       # misaligned queries
    assert lib.kmx_count_lookup2(h, None, _ptr(d_tc), 1000, 47, _ptr(q), None, 10, _ptr(out)) == _lib.E_ARG
    assert lib.kmx_count_lookup2(h, _ptr(d_tk), _ptr(d_tc), 1000, 47, _ptr(q), None, 10, None) == _lib.E_ARG
    assert lib.kmx_count_spectrum(h, _ptr(d_tc), 1000, 1, _ptr(out)) == _lib.E_ARG
    assert lib.kmx_count_spectrum(h, _ptr(d_tc), 1000, 0, _ptr(out)) == _lib.E_ARG


# ---------------------------------------------------------------- the reads form = windows + lookup
def _lookup_reads_check(ctx, orc, table_host, host, n, L, k, offsets=None, shift=0):
    """count_lookup_reads(2) of a batch against a device table: bit-equal to count_lookup(canon, flags) of canonical_windows(2) and
    to the oracle route"""
    tk, tc = table_host
    d_tk, d_tc = ctx.to_device(tk), ctx.to_device(tc)
    buf = ctx.to_device(np.concatenate([np.zeros(shift, np.uint8), host, np.zeros(16, np.uint8)]))
    bases = buf[shift:shift + len(host)]
    d_off = None if offsets is None else ctx.to_device(np.asarray(offsets, np.uint64))
    one = k <= 31
    got = u64((ctx.count_lookup_reads if one else ctx.count_lookup_reads2)(bases, n, L, k, d_tk, d_tc, offsets=d_off))
    w = (ctx.canonical_windows(bases, n, L, k, offsets=d_off, host_offsets=offsets, want=("canon", "flags")) if one else
         ctx.canonical_windows2(bases, n, L, k, offsets=d_off, host_offsets=offsets))
    comp = u64((ctx.count_lookup if one else ctx.count_lookup2)(d_tk, d_tc, k, w["canon"] if one else w["canon"].view(-1, 2), w["flags"]))
    assert got.shape == comp.shape and (got == comp).all(), (k, L, n, shift)
    q, qf = orc_windows(orc, host, n, L, k, offsets)
    expect = host_lookup(tk, tc, q, qf)
    assert got.shape == expect.shape and (got == expect).all(), (k, L, n, shift)
    return got, expect, qf


@pytest.mark.parametrize("k", (5, 13, 21, 31, 33, 47, 64))
def test_lookup_reads_uniform(ctx, orc, k):
    rng = np.random.default_rng(3100 + k)
    for L, n in ((k, 5000), (150, 3000), (300, 700), (1000, 200)):
        a, b = two_batches(rng, n, L)
        table = _thin(*table_of(*orc_windows(orc, a, n, L, k)))
        for shift in (0, 1):                                        # aligned and odd d_bases
            _, expect, qf = _lookup_reads_check(ctx, orc, table, b, n, L, k, shift=shift)
        if L > k:
            _assert_hits_and_misses(expect, qf)
        # dirty and lower-case bytes
        h = dirty(b, rng, 0.10, n, L)
        low = rng.random(n * L) < 0.3
        h[low & (h != ord("N")) & (h != ord(">"))] |= 0x20
        _lookup_reads_check(ctx, orc, table, h, n, L, k, shift=3 if L == 150 else 0)


@pytest.mark.parametrize("k", (13, 31, 35, 47))
@pytest.mark.parametrize("bound", (0, 160, 256, 1000))
def test_lookup_reads_ragged(ctx, orc, k, bound):
    rng = np.random.default_rng(3200 + k + bound)
    hi = {0: 200, 160: 160, 256: 256, 1000: 1000}[bound]
    n = 1500 if hi <= 256 else 300
    lens = rng.integers(0, hi + 1, n)
    lens[::17] = 0                             # empty reads
    lens[5::13] = k - 1                        # reads one base short of a window
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    a = random_reads(rng, int(offsets[-1]))
    b = random_reads(rng, int(offsets[-1]))
    half = int(offsets[n // 2])
    b[:half] = a[:half]                        # the first half of the reads shared
    b[rng.random(len(b)) < 0.002] = ord("N")
    table = _thin(*table_of(*orc_windows(orc, a, n, bound, k, offsets)))
    for shift in (0, 5):                       # (5: misaligned d_bases, the per-read kernels)
        _, expect, qf = _lookup_reads_check(ctx, orc, table, b, n, bound, k, offsets=offsets, shift=shift)
    _assert_hits_and_misses(expect, qf)


@pytest.mark.parametrize("k", (9, 31, 47, 64))
def test_lookup_reads_in_own_table(ctx, k):
    """a batch looked up in ITS OWN table: sum(d_out) == sum(count ** 2), and no valid window answers 0"""
    rng = np.random.default_rng(3300 + k)
    n, L = 20000, 150
    g = random_reads(rng, 50_000)             # reads of a small genome: counts well above 1
    starts = rng.integers(0, len(g) - L + 1, n)
    host = dirty(g[starts[:, None] + np.arange(L)[None, :]].reshape(-1).copy(), rng, 0.05, n, L)
    bases = ctx.to_device(host)
    one = k <= 31
    km, cnt = (ctx.count_canonical if one else ctx.count_canonical2)(bases, n, L, k)
    out = (ctx.count_lookup_reads if one else ctx.count_lookup_reads2)(bases, n, L, k, km, cnt)
    flags = (ctx.canonical_windows(bases, n, L, k, want=("flags",)) if one else ctx.canonical_windows2(bases, n, L, k))["flags"]
    o, f, c = u64(out), flags.cpu().numpy(), u64(cnt)
    assert ((o != 0) == ((f & 1) != 0)).all()
    assert sum(int(x) for x in o.tolist()) == sum(int(x) ** 2 for x in c.tolist())
    # determinism
    again = (ctx.count_lookup_reads if one else ctx.count_lookup_reads2)(bases, n, L, k, km, cnt)
    assert (u64(again) == o).all()


@pytest.mark.parametrize("k", (31, 47))
def test_lookup_reads_work_buffer_cap(ctx, orc, k):
    import torch

    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    rng = np.random.default_rng(3400 + k)
    n, L = 4000, 150
    a, b = two_batches(rng, n, L)
    tk, tc = _thin(*table_of(*orc_windows(orc, a, n, L, k)))
    d_tk, d_tc, bases = ctx.to_device(tk), ctx.to_device(tc), ctx.to_device(b)
    n_win = n * (L - k + 1)
    a256 = lambda x: (x + 255) & ~255
    # the documented working set (kmx.h): 1 byte per window, two-word keys 16 more, each array rounded up to 256
    need = a256(n_win) if k <= 31 else a256(16 * n_win) + a256(n_win)
    fn = ctx.lib.kmx_count_lookup_reads if k <= 31 else ctx.lib.kmx_count_lookup_reads2
    r = _lib.Reads(_ptr(bases), n, L, None)
    out = torch.full((n_win,), -1, dtype=torch.int64, device=ctx.device)
    try:
        ctx.set_work_buffer_limit(need - 1)
        allocs0 = ctx.work_buffer_info()[1]
        st = fn(ctx._h, C.byref(r), None, k, _ptr(d_tk), _ptr(d_tc), len(tc), _ptr(out))
        assert st == _lib.E_NOMEM
        assert ctx.work_buffer_info()[1] == allocs0          # refused before the buffer was touched: nothing ran
        ctx.synchronize()
        assert (out == -1).all()
        ctx.set_work_buffer_limit(need)                      # exactly the documented size: served (without a directory)
        st = fn(ctx._h, C.byref(r), None, k, _ptr(d_tk), _ptr(d_tc), len(tc), _ptr(out))
        assert st == _lib.OK
        q, qf = orc_windows(orc, b, n, L, k)
        assert (u64(out) == host_lookup(tk, tc, q, qf)).all()
    finally:
        ctx.set_work_buffer_limit(0)


@pytest.mark.parametrize("k", (21, 31))
def test_fastq_end_to_end(ctx, orc, k):
    from fastx_cases import fastq_text

    rng = np.random.default_rng(3500 + k)
    t1 = fastq_text(rng, 800, 0, 300)
    t2 = fastq_text(rng, 600, 0, 300)
    # the second image shares its first 300 records with the first: splice the leading lines
    l1, l2 = t1.split(b"\n"), t2.split(b"\n")
    l2[:1200] = l1[:1200]
    t2 = b"\n".join(l2)
    b1, o1 = ctx.fastx_parse(ctx.to_device(t1))
    km, cnt = ctx.count_canonical(b1, int(o1.numel()) - 1, 300, k, offsets=o1)
    b2, o2 = ctx.fastx_parse(ctx.to_device(t2))
    n2 = int(o2.numel()) - 1
    got = u64(ctx.count_lookup_reads(b2, n2, 300, k, km, cnt, offsets=o2))
    e1b, e1o = orc.fastx_parse(t1)
    tk, tc = table_of(*orc_windows(orc, np.asarray(e1b, np.uint8), len(e1o) - 1, 300, k, np.asarray(e1o, np.uint64)))
    e2b, e2o = orc.fastx_parse(t2)
    q, qf = orc_windows(orc, np.asarray(e2b, np.uint8), n2, 300, k, np.asarray(e2o, np.uint64))
    expect = host_lookup(tk, tc, q, qf)
    _assert_hits_and_misses(expect, qf)
    assert got.shape == expect.shape and (got == expect).all()


# ---------------------------------------------------------------- spectrum
BINS = (2, 3, 256, 257, 65536, 2**20)


def _spectrum_check(ctx, counts):
    import torch

    d = ctx.to_device(counts)
    for nb in BINS:
        expect = np.bincount(np.minimum(counts, np.uint64(nb - 1)).astype(np.int64), minlength=nb).astype(np.uint64)
        got = u64(ctx.count_spectrum(d, nb))
        assert got.shape == (nb,) and (got == expect).all(), nb
        assert int(got.sum()) == len(counts)
        bins = torch.zeros(nb, dtype=torch.int64, device=ctx.device)       # accumulation: two calls, the sum
        ctx.count_spectrum(d, nb, out=bins)
        ctx.count_spectrum(d, nb, out=bins)
        assert (u64(bins) == 2 * expect).all(), nb


def test_spectrum_of_tables(ctx):
    rng = np.random.default_rng(41)
    n, L, k = 20000, 150, 31
    host = random_reads(rng, n * L)
    bases = ctx.to_device(host)
    _, cnt = ctx.count_canonical(bases, n, L, k)                           # nearly all singletons
    c = u64(cnt)
    assert (c == 1).mean() > 0.99
    _spectrum_check(ctx, c)
    s = u64(ctx.count_spectrum(cnt, 65536))
    assert int(s[-1]) == 0
    assert sum(i * int(v) for i, v in enumerate(s.tolist())) == ctx.canonical_reduce(bases, n, L, k).n_valid
    poly = rng.random(n) < 0.9                                             # one huge count among singletons
    host.reshape(n, L)[poly] = ord("A")
    for kk, f in ((31, ctx.count_canonical), (47, ctx.count_canonical2)):
        _, cnt = f(ctx.to_device(host), n, L, kk)
        c = u64(cnt)
        assert int(c.max()) > 1_000_000
        _spectrum_check(ctx, c)


def test_spectrum_of_synthetic_counts(ctx):
    rng = np.random.default_rng(42)
    c = np.floor(2.0 ** (rng.random(1_000_000) * 40)).astype(np.uint64)   # log-uniform up to 2^40
    c[:1000] = 0                                                           # (not a count a table holds: bin 0 all the same)
    _spectrum_check(ctx, c)
    _spectrum_check(ctx, np.zeros(0, np.uint64))                           # n = 0
    _spectrum_check(ctx, np.array([5], np.uint64))
    _spectrum_check(ctx, np.full(300_000, U64_MAX, np.uint64))


# ---------------------------------------------------------------- filter
RANGES = ((1, U64_MAX), (2, U64_MAX), (1, 1), (3, 10), (5, 4))


def _genome_table(ctx, rng, k, n=20000, L=150):
    g = random_reads(rng, 100_000)
    starts = rng.integers(0, len(g) - L + 1, n)
    host = g[starts[:, None] + np.arange(L)[None, :]].reshape(-1).copy()
    err = rng.random(len(host)) < 0.01                                     # sequencing errors: singletons
    host[err] = random_reads(rng, int(err.sum()))
    return (ctx.count_canonical if k <= 31 else ctx.count_canonical2)(ctx.to_device(host), n, L, k)


@pytest.mark.parametrize("k", (21, 31, 33, 47, 64))
def test_filter(ctx, k):
    from kmers_amd import _lib

    rng = np.random.default_rng(5100 + k)
    one = k <= 31
    km, cnt = _genome_table(ctx, rng, k)
    hk, hc = u64(km), u64(cnt)
    filt = ctx.count_filter if one else ctx.count_filter2
    for mn, mx in RANGES:
        keep = (hc >= np.uint64(mn)) & (hc <= np.uint64(mx))
        fk, fc = filt(km, cnt, mn, mx)
        assert u64(fk).shape == hk[keep].shape
        assert (u64(fk) == hk[keep]).all() and (u64(fc) == hc[keep]).all(), (k, mn, mx)
    assert 0 < int(((hc >= 3) & (hc <= 10)).sum()) < len(hc)
    # the output is a table: merge(filter(t, 1, 1), filter(t, 2, max)) == t, and it goes into lookup unchanged
    k1, c1 = filt(km, cnt, 1, 1)
    k2, c2 = filt(km, cnt, 2, U64_MAX)
    assert 0 < c1.numel() < cnt.numel()
    mk, mc = (ctx.count_merge if one else ctx.count_merge2)(k1, c1, k2, c2)
    assert (u64(mk) == hk).all() and (u64(mc) == hc).all()
    got = u64((ctx.count_lookup if one else ctx.count_lookup2)(k2, c2, k, km))
    assert (got == np.where(hc >= 2, hc, 0)).all()
    # an empty table
    e = filt(km[:0], cnt[:0], 1, U64_MAX)
    assert e[0].numel() == 0 and e[1].numel() == 0
    with pytest.raises(_lib.KmxError) as ei:
        filt(km, cnt, 1, 1, max_out=int(c1.numel()) - 1)
    assert ei.value.status == _lib.E_NOMEM


@pytest.mark.parametrize("k", (31, 47))
def test_filter_contract(ctx, k):
    import torch

    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    rng = np.random.default_rng(5200 + k)
    w = words(k)
    km, cnt = _genome_table(ctx, rng, k)
    km = km.contiguous().view(-1)
    n = int(cnt.numel())
    hk, hc = u64(km).reshape(n, w), u64(cnt)
    keep = (hc >= 3) & (hc <= 10)
    m = int(keep.sum())
    fn = ctx.lib.kmx_count_filter if w == 1 else ctx.lib.kmx_count_filter2
    sentinel = -0x5A5A5A5A5A5A5A5B
    ok_ = torch.full((w * (m + 8),), sentinel, dtype=torch.int64, device=ctx.device)
    oc = torch.full((m + 8,), sentinel, dtype=torch.int64, device=ctx.device)

    def call(keys, out_k, out_c, max_out):
        got = C.c_uint64(12345)
        st = fn(ctx._h, _ptr(keys), _ptr(cnt), n, 3, 10, _ptr(out_k), _ptr(out_c), max_out, C.byref(got))
        return st, got.value

    assert call(km, ok_, oc, m - 1) == (_lib.E_NOMEM, m)                 # one short: the right count, outputs untouched
    assert (ok_ == sentinel).all() and (oc == sentinel).all()
    assert call(km, None, None, 0) == (_lib.OK, m)                       # count only
    assert call(km, ok_, None, m)[0] == _lib.E_ARG
    assert call(km, None, oc, m)[0] == _lib.E_ARG
    if w == 2:
        assert call(km[1:], ok_, oc, m)[0] == _lib.E_ARG                 # misaligned two-word key arrays
        assert call(km, ok_[1:], oc, m)[0] == _lib.E_ARG
    assert (ok_ == sentinel).all() and (oc == sentinel).all()
    assert call(km, ok_, oc, m) == (_lib.OK, m)                          # exactly the answer; the slots behind it untouched
    assert (u64(ok_[:w * m]).reshape(m, w) == hk[keep]).all() and (u64(oc[:m]) == hc[keep]).all()
    assert (ok_[w * m:] == sentinel).all() and (oc[m:] == sentinel).all()


# the compaction's boundaries: a ballot step (64 entries), a wave's range (4096) and a block's (16384), each minus one, exact, plus one
COMPACT_SIZES = (1, 63, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385, 2 * 16384 + 1)


@pytest.mark.parametrize("w", (1, 2))
def test_filter_compaction_boundaries(ctx, w):
    """Synthetic tables (ascending keys; two-word keys differ in the low word only), counts chosen so that [1, 1] keeps every
    entry, none, only the last, every other one from entry 1 on.  Expected: boolean indexing; the slack behind n_out stays poisoned."""
    import torch

    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    fn = ctx.lib.kmx_count_filter if w == 1 else ctx.lib.kmx_count_filter2
    sentinel = -0x5A5A5A5A5A5A5A5B
    dev = lambda a: torch.from_numpy(a.view(np.int64).reshape(-1)).to(ctx.device)
    for n in COMPACT_SIZES:
        i = np.arange(n, dtype=np.uint64)
        hk = (i + np.uint64(7)).reshape(n, 1)
        if w == 2:
            hk = np.concatenate([hk, np.full((n, 1), 0x1234, np.uint64)], axis=1)   # (low word first)
        hk = np.ascontiguousarray(hk)
        km = dev(hk)
        other = np.uint64(2) + (i % np.uint64(3)) * np.uint64(2**40)               # never 1
        last, odd = i == np.uint64(n - 1), (i & np.uint64(1)) == np.uint64(1)
        for name, keep in (("all", np.ones(n, bool)), ("none", np.zeros(n, bool)), ("last", last), ("odd", odd)):
            hc = np.where(keep, np.uint64(1), other)
            m, cnt = int(keep.sum()), dev(hc)
            ok_ = torch.full((w * (m + 8),), sentinel, dtype=torch.int64, device=ctx.device)
            oc = torch.full((m + 8,), sentinel, dtype=torch.int64, device=ctx.device)
            got = C.c_uint64(12345)
            st = fn(ctx._h, _ptr(km), _ptr(cnt), n, 1, 1, _ptr(ok_), _ptr(oc), m + 8, C.byref(got))
            assert (st, got.value) == (_lib.OK, m), (w, n, name)
            assert (u64(ok_[:w * m]).reshape(m, w) == hk[keep]).all() and (u64(oc[:m]) == hc[keep]).all(), (w, n, name)
            assert (ok_[w * m:] == sentinel).all() and (oc[m:] == sentinel).all(), (w, n, name)


# ---------------------------------------------------------------- at a size the oracle cannot reach
def _big_batches(ctx, n, L, k):
    import torch

    a = ctx.gen_reads(n * L, seed=0xA11CE + k)
    b = ctx.gen_reads(n * L, seed=0xB0B + k)
    b.view(n, L)[::2] = a.view(n, L)[::2]                                 # half of the reads shared
    g = torch.Generator(device=ctx.device).manual_seed(k)
    rows = torch.nonzero(torch.rand(n, device=ctx.device, generator=g) < 0.02).flatten()   # 2 % dirty
    pos = torch.randint(0, L, (rows.numel(),), device=ctx.device, generator=g)
    b[rows * L + pos] = ord("N")
    return a, b


def test_at_size_one_word(ctx):
    """2e6 x 150 bp at k = 31 against the composition of pinned calls: canonical_windows -> torch.searchsorted -> gather -> equal"""
    import torch

    n, L, k = 2_000_000, 150, 31
    a, b = _big_batches(ctx, n, L, k)
    km, cnt = ctx.count_canonical(a, n, L, k)
    got = ctx.count_lookup_reads(b, n, L, k, km, cnt)
    w = ctx.canonical_windows(b, n, L, k, want=("canon", "flags"))
    idx = torch.searchsorted(km, w["canon"]).clamp_(max=km.numel() - 1)    # (keys are below 2^62: signed order = unsigned order)
    expect = torch.where((km[idx] == w["canon"]) & ((w["flags"] & 1) != 0), cnt[idx], torch.zeros_like(cnt[idx]))
    assert torch.equal(got, expect)
    valid = int(((w["flags"] & 1) != 0).sum().item())
    hits = int((got != 0).sum().item())
    assert 10 * hits >= valid and 10 * (valid - hits) >= valid
    assert torch.equal(ctx.count_lookup_reads(b, n, L, k, km, cnt), got)  # determinism
    own = ctx.count_lookup_reads(a, n, L, k, km, cnt)                      # the identity over the whole batch
    assert int(own.sum().item()) == int((cnt * cnt).sum().item())


def test_at_size_two_word(ctx):
    """2e6 x 150 bp at k = 47: the host route on 10^6 windows drawn at random, and the sum-of-squares identity"""
    import torch

    n, L, k = 2_000_000, 150, 47
    a, b = _big_batches(ctx, n, L, k)
    km, cnt = ctx.count_canonical2(a, n, L, k)
    got = ctx.count_lookup_reads2(b, n, L, k, km, cnt)
    w = ctx.canonical_windows2(b, n, L, k)
    g = torch.Generator(device=ctx.device).manual_seed(7)
    pick = torch.randint(0, got.numel(), (1_000_000,), device=ctx.device, generator=g)
    q = u64(w["canon"].view(-1, 2)[:, 0][pick]), u64(w["canon"].view(-1, 2)[:, 1][pick])
    qf = w["flags"][pick].cpu().numpy()
    tk = np.stack([u64(km[:, 0].contiguous()), u64(km[:, 1].contiguous())], axis=1)
    expect = host_lookup(tk, u64(cnt), np.stack(q, axis=1), qf)
    _assert_hits_and_misses(expect, qf)
    assert (u64(got[pick]) == expect).all()
    del w
    own = ctx.count_lookup_reads2(a, n, L, k, km, cnt)
    assert int(own.sum().item()) == int((cnt * cnt).sum().item())
