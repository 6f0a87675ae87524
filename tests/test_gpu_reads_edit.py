"""A new batch of reads from an old one on the GPU: kmx_reads_select and kmx_reads_gather (kmx_reads_edit.hip), and what the Python
layer builds on them (Context.reads_select, reads_gather, reads_partition, count_select_reads(2), ReadPaths.read_components).

Every comparison is equality of every output byte, offset and index word with the host reference tests/reads_np.py (pinned against
Python slicing in tests/test_reads_np.py): there is no tolerance anywhere.  The raw calls go through `run_select` / `run_gather`, which
hand the ABI buffers that are longer than the result and filled with a sentinel, and look at every byte and word behind the result.
Every family asserts of its own input that it holds what it is there for."""
import ctypes as C

import numpy as np
import pytest

from tests import reads_np
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import random_reads, u64
from tests.reads_np import span_word
from tests.reads_dev import SENT, SENT_WORD, dev_bytes, dev_words, ptr

pytestmark = pytest.mark.gpu

OK, E_ARG, E_NOMEM = 0, 1, 6
GUARD = 64           # sentinel bytes behind d_out_bases


class Batch:
    """a batch of reads on the host and on the device; offsets None = uniform reads of read_len bases"""

    def __init__(self, ctx, bases, n_reads, read_len=0, offsets=None, shift=0):
        from kmers_amd._lib import Reads

        self.ctx, self.h_bases, self.n, self.read_len, self.h_off = ctx, np.asarray(bases, np.uint8), int(n_reads), int(read_len), offsets
        self.d_bases = dev_bytes(ctx, self.h_bases, shift)
        self.d_off = dev_words(ctx, offsets)
        self.reads = Reads(self.d_bases.data_ptr() if self.n else None, self.n, self.read_len, self.d_off.data_ptr() if offsets is not None else None)

    def args(self):
        return (self.d_bases, self.n, self.read_len)


def ragged(ctx, lens, rng, first=0, shift=0):
    lens = np.asarray(lens, np.int64)
    offsets = (np.concatenate([[0], np.cumsum(lens)]) + first).astype(np.uint64)
    bases = np.concatenate([np.full(first, ord("."), np.uint8), random_reads(rng, int(lens.sum()))])
    return Batch(ctx, bases, len(lens), 0, offsets, shift)


def _span_dev(ctx, span, stride):
    """span words on the device, `stride` words apart (the words between are poison)"""
    if span is None:
        return None, 0
    a = np.full(max(len(span) * stride, 1), 0xDEADBEEFDEADBEEF, np.uint64)
    a[:len(span) * stride:stride] = span
    return dev_words(ctx, a), stride


def run_select(b, keep=None, span=None, span_k=0, min_len=0, stride=1, out_shift=0, want_index=True):
    """kmx_reads_select through the raw ABI: a count-only call, then the write into guarded buffers; everything is compared with
    the reference -> (out bases, out offsets, index) on the host, and the device tensors for pointer arithmetic"""
    import torch

    ctx = b.ctx
    want_b, want_o, want_i = reads_np.select_np(b.h_bases, b.n, b.read_len, b.h_off, keep=keep, span=span, span_k=span_k, min_len=min_len)
    d_keep = dev_bytes(ctx, np.asarray(keep, np.uint8)) if keep is not None else None
    d_span, stride = _span_dev(ctx, span, stride)
    nr, nb = C.c_uint64(99), C.c_uint64(99)
    head = (ctx._h, C.byref(b.reads), ptr(d_keep), ptr(d_span), stride, span_k, min_len)
    st = ctx.lib.kmx_reads_select(*head, None, None, None, 0, 0, C.byref(nr), C.byref(nb))
    assert st == OK and (nr.value, nb.value) == (len(want_i), len(want_b)), (st, nr.value, nb.value, len(want_i), len(want_b))
    n_out, n_bases = nr.value, nb.value
    raw = torch.full((n_bases + GUARD + 32,), SENT, dtype=torch.uint8, device=ctx.device)
    out = raw[out_shift:out_shift + n_bases + GUARD]
    off = torch.full((n_out + 2,), SENT_WORD, dtype=torch.int64, device=ctx.device)
    idx = torch.full((n_out + 1,), SENT_WORD, dtype=torch.int64, device=ctx.device)
    nr, nb = C.c_uint64(99), C.c_uint64(99)
    st = ctx.lib.kmx_reads_select(*head, ptr(out), ptr(off), ptr(idx) if want_index else None, n_out, n_bases, C.byref(nr), C.byref(nb))
    assert st == OK and (nr.value, nb.value) == (n_out, n_bases)
    h_raw, h_off, h_idx = raw.cpu().numpy(), u64(off), u64(idx)
    h_out = h_raw[out_shift:out_shift + n_bases]
    if b.n:
        assert np.array_equal(h_out, want_b), "bytes"
        assert np.array_equal(h_off[:n_out + 1], want_o), "offsets"
    else:
        assert (h_off == np.uint64(SENT_WORD & (2**64 - 1))).all()          # a no-op: not even offsets[0]
    assert (h_raw[:out_shift] == SENT).all() and (h_raw[out_shift + n_bases:] == SENT).all(), "a byte outside the result was written"
    assert h_off[n_out + 1] == np.uint64(SENT_WORD & (2**64 - 1)), "the word after the offsets was written"
    if want_index:
        assert np.array_equal(h_idx[:n_out], want_i), "index"
    else:
        assert (h_idx[:n_out] == np.uint64(SENT_WORD & (2**64 - 1))).all()
    assert h_idx[n_out] == np.uint64(SENT_WORD & (2**64 - 1)), "the word after the index was written"
    return h_out, h_off[:n_out + 1], want_i, out


def run_gather(b, index, span=None, span_k=0, stride=1, out_shift=0):
    import torch

    ctx = b.ctx
    index = np.asarray(index, np.uint64)
    want_b, want_o = reads_np.gather_np(b.h_bases, b.n, b.read_len, index, b.h_off, span=span, span_k=span_k)
    d_index = dev_words(ctx, index) if len(index) else None
    d_span, stride = _span_dev(ctx, span, stride)
    nb = C.c_uint64(99)
    head = (ctx._h, C.byref(b.reads), ptr(d_index), len(index), ptr(d_span), stride, span_k)
    st = ctx.lib.kmx_reads_gather(*head, None, None, 0, C.byref(nb))
    assert st == OK and nb.value == len(want_b), (st, nb.value, len(want_b))
    n_bases = nb.value
    raw = torch.full((n_bases + GUARD + 32,), SENT, dtype=torch.uint8, device=ctx.device)
    out = raw[out_shift:out_shift + n_bases + GUARD]
    off = torch.full((len(index) + 2,), SENT_WORD, dtype=torch.int64, device=ctx.device)
    nb = C.c_uint64(99)
    st = ctx.lib.kmx_reads_gather(*head, ptr(out), ptr(off), n_bases, C.byref(nb))
    assert st == OK and nb.value == n_bases
    h_raw, h_off = raw.cpu().numpy(), u64(off)
    sent = np.uint64(SENT_WORD & (2**64 - 1))
    if len(index):
        assert np.array_equal(h_raw[out_shift:out_shift + n_bases], want_b), "bytes"
        assert np.array_equal(h_off[:len(index) + 1], want_o), "offsets"
    else:
        assert (h_off == sent).all()
    assert (h_raw[:out_shift] == SENT).all() and (h_raw[out_shift + n_bases:] == SENT).all(), "a byte outside the result was written"
    assert h_off[len(index) + 1] == sent, "the word after the offsets was written"
    return h_raw[out_shift:out_shift + n_bases], h_off[:len(index) + 1]


# ---------------------------------------------------------------- short ragged reads: several reads in one 16-byte piece
def _short_lens(rng, n=3000):
    lens = rng.integers(0, 41, n)
    short = rng.random(n) < 0.5
    lens[short] = rng.integers(0, 16, int(short.sum()))
    for at, run in ((100, 40), (1500, 7), (2990, 10)):      # runs of consecutive empty reads, one at the batch's end
        lens[at:at + run] = 0
    return lens


def _random_spans(rng, lens):
    """spans in bases: inside, past the end, start == L, start > L, zero length, 32-bit extremes"""
    n = len(lens)
    start = (rng.random(n) * (lens + 1)).astype(np.int64)
    length = (rng.random(n) * (lens + 2)).astype(np.int64)
    far = rng.random(n) < 0.15
    start[far] = lens[far] + rng.integers(0, 3, int(far.sum()))
    long_ = rng.random(n) < 0.2
    length[long_] = rng.integers(0, 1000, int(long_.sum()))
    start[::97], length[::97] = 0xFFFFFFFF, 0xFFFFFFFF
    length[5::101] = 0xFFFFFFFF
    return np.array([span_word(s, n_) for s, n_ in zip(start, length)], np.uint64)


@pytest.mark.parametrize("shift", (0, 1, 3, 7))
@pytest.mark.parametrize("first", (0, 5))
def test_short_ragged_reads(ctx, first, shift):
    rng = np.random.default_rng(9100 + 16 * first + shift)
    lens = _short_lens(rng)
    assert (lens <= 15).mean() > 0.5 and (lens == 0).sum() > 100
    b = ragged(ctx, lens, rng, first=first, shift=shift)
    assert b.d_bases.data_ptr() % 16 == shift
    span = _random_spans(rng, lens)
    seen = set()
    for density, keep in (("none", np.zeros(len(lens), np.uint8)), ("half", (rng.random(len(lens)) < 0.5).astype(np.uint8) * 3),
                          ("all", np.ones(len(lens), np.uint8))):
        for sp, stride in ((None, 1), (span, 1), (span, 3)):
            out_shift = int(rng.integers(0, 16))
            _, off, idx, d_out = run_select(b, keep=keep, span=sp, span_k=0, stride=stride, out_shift=out_shift)
            if density == "none":
                assert len(idx) == 0 and off.tolist() == [0]
                continue
            # the relative misalignment of every non-empty output read: source address against destination address, mod 16
            src, ln = reads_np.clips(b.n, 0, b.h_off, sp, 0)
            i = idx.astype(np.int64)
            rel = (b.d_bases.data_ptr() + src[i] - (d_out.data_ptr() + off[:-1].astype(np.int64))) % 16
            seen |= set(rel[ln[i] > 0].tolist())
    assert seen == set(range(16)), seen
    # spans in windows: the same words read with span_k = 4
    run_select(b, keep=None, span=span, span_k=4, min_len=0, out_shift=5)


def test_one_read_spans_many_blocks(ctx):
    """one read of 100 000 bases among short ones: 7 blocks of the copy lie inside it; and the global search behind the staged reads,
    which a block needs when its 16 KiB hold more than 512 reads"""
    rng = np.random.default_rng(9200)
    lens = np.concatenate([rng.integers(0, 30, 700), [100_000], rng.integers(0, 12, 5000), [0, 0, 3]])
    b = ragged(ctx, lens, rng, first=3, shift=1)
    run_select(b, out_shift=9)
    span = np.array([span_word(1, max(int(v) - 2, 0)) for v in lens], np.uint64)
    run_select(b, span=span, min_len=1, out_shift=0)
    run_gather(b, rng.permutation(len(lens)), out_shift=2)


def test_short_reads_over_several_blocks(ctx):
    """12 000 short reads: several blocks of the copy, each with more reads than it stages, so that pieces in one block are found
    both among the staged offsets and behind them"""
    rng = np.random.default_rng(9250)
    lens = _short_lens(rng, 12_000)
    assert lens.sum() > 3 * 65_536 - 40_000
    b = ragged(ctx, lens, rng, first=5, shift=3)
    run_select(b, out_shift=7)
    run_select(b, keep=(rng.random(len(lens)) < 0.5).astype(np.uint8), span=_random_spans(rng, lens), out_shift=12)


@pytest.mark.parametrize("n_bytes", (1, 15, 16, 17, 4097))
def test_output_lengths(ctx, n_bytes):
    """the batch's first and last piece, alone and together: every alignment of a short output"""
    rng = np.random.default_rng(9300 + n_bytes)
    lens = np.array([0, 3, 5000, 0, 11])
    b = ragged(ctx, lens, rng, first=2, shift=3)
    keep = np.array([1, 0, 1, 1, 0], np.uint8)
    span = np.array([span_word(0, 9), span_word(0, 9), span_word(7, n_bytes), span_word(0, 0), span_word(0, 9)], np.uint64)
    for out_shift in (0, 1, 15, 8):
        out, off, idx, _ = run_select(b, keep=keep, span=span, out_shift=out_shift)
        assert len(out) == n_bytes and off.tolist() == [0, 0, n_bytes, n_bytes] and idx.tolist() == [0, 2, 3]
    # the same length made of several reads
    parts = np.array([1] * min(n_bytes, 20) + [n_bytes - min(n_bytes, 20)])
    b = ragged(ctx, parts, rng, shift=7)
    out, _, _, _ = run_select(b, out_shift=13)
    assert len(out) == n_bytes


# ---------------------------------------------------------------- uniform reads, spans from count_read_stats
def test_uniform_reads_trimmed_by_read_stats(ctx):
    import torch

    from kmers_amd._lib import RS_N_SOLID, RS_N_VALID, RS_SPAN
    from kmers_amd.api import read_stats_span

    rng = np.random.default_rng(9400)
    n, L, k = 1000, 150, 31
    host = random_reads(rng, n * L).reshape(n, L)
    for i in range(n // 2, n):                      # the second half: a prefix or a suffix of a read of the first half, then noise
        a = int(rng.integers(0, L + 1))
        if i % 2:
            host[i, :a] = host[i - n // 2, :a]
        else:
            host[i, a:] = host[i - n // 2, a:]
        if i % 50 == 0:
            host[i, L // 2] = ord("N")
    host = host.reshape(-1)
    d = ctx.to_device(host)
    kmers, counts = ctx.count_canonical(d[:n // 2 * L], n // 2, L, k)
    stats = ctx.count_read_stats(d, n, L, k, kmers, counts, solid_min=1)
    first, end = read_stats_span(stats, k)
    first, end = first.cpu().numpy(), end.cpu().numpy()
    assert ((end - first) == L).sum() >= n // 2 and (end == 0).sum() > 5 and ((end - first > 0) & (end - first < L)).sum() > 300
    batch = ctx.reads_select(d, n, L, span=stats[:, RS_SPAN], span_k=k, min_len=k, index=True)
    kept = np.nonzero(end - first >= k)[0]
    assert batch.n_reads == len(kept) and np.array_equal(batch.index.cpu().numpy(), kept)
    want = np.concatenate([host[r * L + first[r]:r * L + end[r]] for r in kept])
    assert np.array_equal(batch.bases.cpu().numpy(), want)
    assert np.array_equal(batch.offsets.cpu().numpy(), np.concatenate([[0], np.cumsum((end - first)[kept])]))
    # and through the raw call with the reference, the stats rows as they lie: stride KMX_RS_WORDS
    b = Batch(ctx, host, n, L)
    span = u64(stats)[:, RS_SPAN].copy()
    out, off, idx, _ = run_select(b, span=span, span_k=k, min_len=k, stride=8)
    assert np.array_equal(out, want) and np.array_equal(idx, kept.astype(np.uint64))
    # every kept read is solid from end to end
    assert batch.max_len() == int((end - first).max())
    again = ctx.count_read_stats(batch.bases, batch.n_reads, batch.max_len(), k, kmers, counts, solid_min=1, offsets=batch.offsets).cpu().numpy()
    clean = np.array([np.isin(want[a:e], np.frombuffer(b"ACGT", np.uint8)).all() for a, e in zip(off[:-1].astype(np.int64), off[1:].astype(np.int64))])
    assert clean.sum() > 500
    assert (again[clean, RS_N_SOLID] == again[clean, RS_N_VALID]).all() and (again[clean, RS_N_VALID] > 0).all()
    assert torch.equal(stats, ctx.count_read_stats(d, n, L, k, kmers, counts, solid_min=1))   # (the source's rows are untouched)


# ---------------------------------------------------------------- conventions
def _small(ctx):
    rng = np.random.default_rng(9500)
    lens = np.array([10, 0, 4, 1, 0, 0, 25, 2, 16, 31])
    return ragged(ctx, lens, rng, first=4, shift=1), lens


def test_conventions(ctx):
    import torch

    b, lens = _small(ctx)
    sent = lambda n, dt: torch.full((n,), SENT if dt == torch.uint8 else SENT_WORD, dtype=dt, device=ctx.device)
    out, off, idx = sent(200, torch.uint8), sent(16, torch.int64), sent(16, torch.int64)
    nr, nb = C.c_uint64(99), C.c_uint64(99)
    sel = lambda *tail: ctx.lib.kmx_reads_select(ctx._h, C.byref(b.reads), None, None, 0, 0, 0, *tail, C.byref(nr), C.byref(nb))
    untouched = lambda: bool((out == SENT).all() and (off == SENT_WORD).all() and (idx == SENT_WORD).all())
    # count only: the counts, nothing else
    assert sel(None, None, None, 0, 0) == OK and (nr.value, nb.value) == (10, int(lens.sum()))
    # one byte, one read short: KMX_E_NOMEM, the counts set, nothing written
    nr.value = nb.value = 99
    assert sel(ptr(out), ptr(off), ptr(idx), 10, int(lens.sum()) - 1) == E_NOMEM and (nr.value, nb.value) == (10, int(lens.sum())) and untouched()
    assert sel(ptr(out), ptr(off), ptr(idx), 9, int(lens.sum())) == E_NOMEM and untouched()
    # exactly one of the two outputs
    assert sel(ptr(out), None, None, 10, 200) == E_ARG and sel(None, ptr(off), None, 10, 200) == E_ARG and untouched()
    # a span array without a stride
    d_span = dev_words(ctx, np.zeros(10, np.uint64))
    assert ctx.lib.kmx_reads_select(ctx._h, C.byref(b.reads), None, ptr(d_span), 0, 0, 0, ptr(out), ptr(off), None, 10, 200, C.byref(nr), C.byref(nb)) == E_ARG
    assert ctx.lib.kmx_reads_gather(ctx._h, C.byref(b.reads), ptr(d_span), 3, ptr(d_span), 0, 0, ptr(out), ptr(off), 200, C.byref(nb)) == E_ARG
    assert ctx.lib.kmx_reads_gather(ctx._h, C.byref(b.reads), ptr(d_span), 3, None, 0, 0, ptr(out), None, 200, C.byref(nb)) == E_ARG
    assert untouched()
    # the output over the source
    assert ctx.lib.kmx_reads_select(ctx._h, C.byref(b.reads), None, None, 0, 0, 0, C.c_void_p(b.d_bases.data_ptr() + 8), ptr(off), None, 10, 200,
                                    C.byref(nr), C.byref(nb)) == E_ARG and untouched()
    # gather: a byte short
    nb.value = 99
    assert ctx.lib.kmx_reads_gather(ctx._h, C.byref(b.reads), ptr(dev_words(ctx, np.array([6, 6], np.uint64))), 2, None, 0, 0, ptr(out), ptr(off), 49,
                                    C.byref(nb)) == E_NOMEM and nb.value == 50 and untouched()
    # no reads: a no-op with zero counts
    e = Batch(ctx, np.zeros(0, np.uint8), 0, 0, np.zeros(1, np.uint64))
    run_select(e)
    e = Batch(ctx, np.zeros(0, np.uint8), 0, 150, None)
    run_select(e)
    run_gather(e, [0, 1, 5])          # every index is past the end: three empty reads
    run_gather(b, [])


def test_min_len_boundary_and_empty_reads(ctx):
    b, lens = _small(ctx)
    for min_len in (0, 1, 2, 3, 4, 5, 16, 17, 25, 26, 31, 32):
        _, _, idx, _ = run_select(b, min_len=min_len, want_index=(min_len % 2 == 0))
        assert idx.tolist() == [i for i, v in enumerate(lens) if v >= min_len]      # exactly min_len stays, one shorter goes
    keep = np.array([0, 1, 1, 0, 1, 1, 0, 0, 0, 1], np.uint8)
    _, off, idx, _ = run_select(b, keep=keep)                                       # min_len == 0 keeps the empty reads 1, 4, 5
    assert idx.tolist() == [1, 2, 4, 5, 9] and off.tolist() == [0, 0, 4, 4, 4, 35]
    span = np.array([span_word(3, 0)] * 10, np.uint64)
    _, off, idx, _ = run_select(b, span=span)                                       # every clip empty, every read kept
    assert len(idx) == 10 and off.tolist() == [0] * 11
    _, _, idx, _ = run_select(b, span=span, min_len=1)
    assert len(idx) == 0


# ---------------------------------------------------------------- gather
def test_gather(ctx):
    rng = np.random.default_rng(9600)
    lens = _short_lens(rng, 2000)
    lens[77] = 5000
    b = ragged(ctx, lens, rng, first=5, shift=3)
    span = _random_spans(rng, lens)
    perm = rng.permutation(len(lens))
    run_gather(b, perm, out_shift=4)
    run_gather(b, perm, span=span, stride=2, out_shift=11)
    run_gather(b, rng.integers(0, len(lens), 5000), out_shift=1)                    # repeats
    run_gather(b, [77, 77, 77, 0, 77])
    index = rng.integers(0, len(lens), 1000).astype(np.uint64)
    index[::7] = len(lens) + rng.integers(0, 5, len(index[::7])).astype(np.uint64)  # past the end: empty reads
    index[3], index[10] = 2**64 - 1, 2**40
    out, off = run_gather(b, index, span=span, span_k=3)
    assert (np.diff(off.astype(np.int64))[::7] == 0).all()
    run_gather(b, [])
    g_out, g_off = run_gather(b, np.arange(len(lens)), span=span, out_shift=6)      # arange = select without keep
    s_out, s_off, _, _ = run_select(b, span=span, out_shift=6)
    assert np.array_equal(g_out, s_out) and np.array_equal(g_off, s_off)
    # uniform reads
    u = Batch(ctx, random_reads(rng, 300 * 37), 300, 37, None, shift=7)
    run_gather(u, rng.integers(0, 310, 700), span=_random_spans(rng, np.full(300, 37)), out_shift=3)


def test_python_layer_matches_raw(ctx):
    import torch

    rng = np.random.default_rng(9700)
    lens = _short_lens(rng, 1500)
    b = ragged(ctx, lens, rng)
    keep = rng.random(len(lens)) < 0.6
    span = _random_spans(rng, lens)
    rows = np.full((len(lens), 8), 0xDEADBEEF, np.uint64)
    rows[:, 7] = span
    d_rows = dev_words(ctx, rows)
    got = ctx.reads_select(*b.args(), keep=torch.from_numpy(keep).to(ctx.device), span=d_rows[:, 7], min_len=2, offsets=b.d_off, index=True)
    assert d_rows[:, 7].data_ptr() == d_rows.data_ptr() + 56 and not d_rows[:, 7].is_contiguous()     # a view: no copy was made
    wb, wo, wi = reads_np.select_np(b.h_bases, b.n, 0, b.h_off, keep=keep, span=span, min_len=2)
    assert np.array_equal(got.bases.cpu().numpy(), wb) and np.array_equal(u64(got.offsets), wo) and np.array_equal(u64(got.index), wi)
    assert got.n_reads == len(wi) and got.max_len() == int(np.diff(wo.astype(np.int64)).max())
    none = ctx.reads_select(*b.args(), keep=torch.zeros(len(lens), dtype=torch.uint8, device=ctx.device), offsets=b.d_off)
    assert none.n_reads == 0 and none.bases.numel() == 0 and none.offsets.tolist() == [0] and none.index is None and none.max_len() == 0
    index = torch.from_numpy(rng.integers(0, len(lens) + 3, 800)).to(ctx.device)
    g = ctx.reads_gather(*b.args(), index, span=d_rows[:, 7], offsets=b.d_off)
    wb, wo = reads_np.gather_np(b.h_bases, b.n, 0, u64(index), b.h_off, span=span)
    assert np.array_equal(g.bases.cpu().numpy(), wb) and np.array_equal(u64(g.offsets), wo) and g.n_reads == 800
    # the result goes straight into another call
    twice = ctx.reads_select(got.bases, got.n_reads, got.max_len(), offsets=got.offsets)
    assert torch.equal(twice.bases, got.bases) and torch.equal(twice.offsets, got.offsets)


# ---------------------------------------------------------------- partition
@pytest.mark.parametrize("n_labels", (1, 500))
def test_partition(ctx, n_labels):
    import torch

    rng = np.random.default_rng(9800 + n_labels)
    lens = _short_lens(rng, 2500)
    b = ragged(ctx, lens, rng, first=5)
    values = np.sort(rng.choice(10_000, n_labels, replace=False)) * 3 + 1                  # labels with gaps
    which = np.arange(len(lens)) % n_labels
    rng.shuffle(which)
    labels = values[which]
    spare = np.setdiff1d(np.arange(len(lens)), np.unique(which, return_index=True)[1])     # every label keeps its first read
    labels[rng.choice(spare, 500, replace=False)] = -rng.integers(1, 9, 500)               # negatives: dropped
    assert (labels < 0).sum() > 100 and len(np.unique(labels[labels >= 0])) == n_labels
    g = ctx.reads_partition(*b.args(), torch.from_numpy(labels).to(ctx.device), offsets=b.d_off)
    wb, wo, wi, wd, wg = reads_np.partition_np(b.h_bases, b.n, 0, labels, b.h_off)
    assert np.array_equal(g.batch.bases.cpu().numpy(), wb) and np.array_equal(u64(g.batch.offsets), wo) and np.array_equal(u64(g.batch.index), wi)
    assert np.array_equal(g.labels.cpu().numpy(), wd) and np.array_equal(g.group_offsets.cpu().numpy(), wg) and g.n_groups == n_labels
    # the groups concatenate to a stable sort of the kept reads
    idx, go = g.batch.index.cpu().numpy(), g.group_offsets.cpu().numpy()
    for q in range(g.n_groups):
        members = idx[go[q]:go[q + 1]]
        assert (labels[members] == wd[q]).all() and (np.diff(members) > 0).all()
    assert sorted(idx.tolist()) == np.nonzero(labels >= 0)[0].tolist()


def test_read_components_split_two_genomes(ctx):
    import torch

    rng = np.random.default_rng(9900)
    k = 21
    genomes = [random_reads(rng, 2000), random_reads(rng, 2000)]
    reads, origin = [], []
    for i in range(400):
        g = i % 2 if i % 5 else int(rng.integers(0, 2))
        L = int(rng.integers(40, 121))
        a = int(rng.integers(0, 2000 - L + 1))
        reads.append(genomes[g][a:a + L])
        origin.append(g)
    reads.append(np.frombuffer(b"ACGTNNNN", np.uint8))          # a read without a window: label -1
    origin.append(-1)
    origin = np.array(origin)
    lens = np.array([len(r) for r in reads])
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    b = Batch(ctx, np.concatenate(reads), len(reads), 0, offsets)
    kmers, counts = ctx.count_canonical(ctx.to_device(np.concatenate(genomes)), 2, 0, k, offsets=ctx.to_device(np.array([0, 2000, 4000], np.uint64)))
    adj = ctx.count_adjacency(kmers, counts, k, 1, flips=True, neighbors=True)
    un = ctx.count_unitigs(kmers, counts, k, 1, adjacency=adj)
    n = int(counts.numel())
    place = ctx.count_unitig_index(un, n)
    links = ctx.count_unitig_links(un, adj, n, place=place)
    comp = ctx.count_unitig_components(un, links)
    paths = ctx.count_read_paths(b.d_bases, b.n, int(lens.max()), k, kmers, un, place=place, offsets=b.d_off)
    labels = paths.read_components(comp, b.n)
    h_labels = labels.cpu().numpy()
    assert h_labels[-1] == -1 and (h_labels[:-1] >= 0).all()
    # the reference of read_components: the smallest id over the read's segments
    seg_read, seg_id = paths.read.cpu().numpy(), paths.components(comp).cpu().numpy()
    for r in (0, 1, 17, 399):
        assert h_labels[r] == seg_id[seg_read == r].min()
    groups = ctx.reads_partition(*b.args(), labels, offsets=b.d_off)
    assert groups.n_groups == 2, groups.labels                  # two random genomes share no 21-mer
    idx, go = groups.batch.index.cpu().numpy(), groups.group_offsets.cpu().numpy()
    for q in range(2):
        members = idx[go[q]:go[q + 1]]
        assert len(set(origin[members].tolist())) == 1          # every read of one genome in one group
    assert set(origin[idx[:go[1]]].tolist()) != set(origin[idx[go[1]:]].tolist()) and len(idx) == 400
    wb, wo, wi, _, _ = reads_np.partition_np(b.h_bases, b.n, 0, h_labels, b.h_off)
    assert np.array_equal(groups.batch.bases.cpu().numpy(), wb) and np.array_equal(u64(groups.batch.offsets), wo)


# ---------------------------------------------------------------- count_select_reads
@pytest.mark.parametrize("k", (31, 41))
def test_count_select_reads(ctx, k):
    from kmers_amd._lib import RS_MEDIAN, RS_SPAN

    rng = np.random.default_rng(10_000 + k)
    n, L = 600, 120
    genome = random_reads(rng, 3000)
    clean = np.stack([genome[a:a + L] for a in rng.integers(0, 3000 - L + 1, n)])
    noisy = clean.copy()
    flip = rng.random(noisy.shape) < 0.01
    noisy[flip] = np.frombuffer(b"CAGT", np.uint8)[(noisy[flip] >> 1) & 3]         # A C T G -> C A G T: another base
    assert (noisy != clean).sum() > 300
    noisy[::40] = random_reads(rng, len(noisy[::40]) * L).reshape(-1, L)           # reads from elsewhere: median 0
    d_clean, d_noisy = ctx.to_device(clean.reshape(-1)), ctx.to_device(noisy.reshape(-1))
    count, select = (ctx.count_canonical, ctx.count_select_reads) if k <= 31 else (ctx.count_canonical2, ctx.count_select_reads2)
    kmers, counts = count(d_clean, n, L, k)
    host = noisy.reshape(-1)
    for min_median, max_median, trim in ((2, 2**64 - 1, True), (1, 17, True), (3, 2**64 - 1, False)):
        batch, stats = select(d_noisy, n, L, k, kmers, counts, solid_min=2, min_median=min_median, max_median=max_median, trim=trim)
        st = u64(stats)
        med, w = st[:, RS_MEDIAN], st[:, RS_SPAN]
        start, wins = (w & np.uint64(0xFFFFFFFF)).astype(np.int64), (w >> np.uint64(32)).astype(np.int64)
        ln = np.where(wins > 0, wins + k - 1, 0) if trim else np.full(n, L)
        start = start if trim else np.zeros(n, np.int64)
        keep = (med >= np.uint64(min_median)) & (med <= np.uint64(max_median)) & (ln >= k)     # the median test, on the host
        assert 50 < keep.sum() < n
        idx = batch.index.cpu().numpy()
        assert np.array_equal(idx, np.nonzero(keep)[0]) and batch.n_reads == int(keep.sum())
        off, out = batch.offsets.cpu().numpy(), batch.bases.cpu().numpy()
        for j, r in enumerate(idx):                                                # a substring of its source read at the reported span
            assert np.array_equal(out[off[j]:off[j + 1]], host[r * L + start[r]:r * L + start[r] + ln[r]])
        if trim:
            assert ((ln[idx] < L).sum() > 20) and (ln[idx] >= k).all()


def test_two_calls_give_identical_bytes(ctx):
    import torch

    rng = np.random.default_rng(10_100)
    lens = _short_lens(rng, 3000)
    lens[1234] = 40_000
    b = ragged(ctx, lens, rng, first=5, shift=3)
    keep = torch.from_numpy((rng.random(len(lens)) < 0.7).astype(np.uint8)).to(ctx.device)
    span = dev_words(ctx, _random_spans(rng, lens))
    a1 = ctx.reads_select(*b.args(), keep=keep, span=span, offsets=b.d_off, index=True)
    a2 = ctx.reads_select(*b.args(), keep=keep, span=span, offsets=b.d_off, index=True)
    assert torch.equal(a1.bases, a2.bases) and torch.equal(a1.offsets, a2.offsets) and torch.equal(a1.index, a2.index)
    index = torch.from_numpy(rng.integers(0, len(lens), 4000)).to(ctx.device)
    g1 = ctx.reads_gather(*b.args(), index, span=span, offsets=b.d_off)
    g2 = ctx.reads_gather(*b.args(), index, span=span, offsets=b.d_off)
    assert torch.equal(g1.bases, g2.bases) and torch.equal(g1.offsets, g2.offsets)
