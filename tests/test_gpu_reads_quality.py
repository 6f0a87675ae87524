"""kmx_reads_quality on the GPU (kmx_reads_quality.hip) and what the Python layer builds on it (Context.reads_quality,
reads_quality_filter, expected_errors).

Every comparison is equality of every masked byte and every row word with the host reference tests/quality_np.py (pinned against
brute force in tests/test_quality_np.py): there is no tolerance anywhere.  The raw call goes through `run`, which hands the ABI a
d_masked with sentinel bytes before, behind and between the reads and a d_rows with sentinel words around it, and looks at all of
them afterwards."""
import ctypes as C

import numpy as np
import pytest

from tests import quality_np as Q
from tests import reads_np
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import u64
from tests.reads_dev import SENT, SENT_WORD, dev_bytes, dev_words, ptr

pytestmark = pytest.mark.gpu

OK, E_ARG = 0, 1
GUARD = 64
GW = 8                            # sentinel words on either side of d_rows
BASE_ALPHA = np.frombuffer(b"ACGTACGTACGTACGTacgtN", np.uint8)


def make_batch(rng, lens, first=0, qlo=33, qhi=33 + 41):
    """ragged reads: (bases, quals, offsets); the `first` bytes before the batch are '.' / 0xFF"""
    lens = np.asarray(lens, np.int64)
    off = (np.concatenate([[0], np.cumsum(lens)]) + first).astype(np.uint64)
    n = int(lens.sum())
    bases = np.concatenate([np.full(first, ord("."), np.uint8), rng.choice(BASE_ALPHA, n).astype(np.uint8)])
    quals = np.concatenate([np.full(first, 0xFF, np.uint8), rng.integers(qlo, qhi + 1, n).astype(np.uint8)])
    return bases, quals, off


def run(ctx, bases, quals, n, read_len=0, off=None, bshift=0, qshift=0, mshift=0, phred=33, min_q=0, trim_q=0, k=0, weights=None,
        want=None, inplace=False, mask=True, rows=True):
    """kmx_reads_quality through the raw ABI into guarded buffers -> (masked bytes of the whole layout, rows uint64[n, 8]), both
    compared with the reference `want` (computed here unless given)"""
    import torch
    from kmers_amd._lib import Reads

    if want is None:
        want = Q.reads_quality_np(bases, quals, n, read_len, off, phred, min_q, trim_q, k, weights)
    d_b = dev_bytes(ctx, bases, bshift)
    d_q = dev_bytes(ctx, quals, qshift)
    d_off = dev_words(ctx, off)
    d_w = dev_words(ctx, weights)
    total = len(bases)
    mbuf = torch.full((GUARD + mshift + total + GUARD,), SENT, dtype=torch.uint8, device=ctx.device)
    d_m = d_b if inplace else mbuf[GUARD + mshift:GUARD + mshift + total]
    rbuf = torch.full((2 * GW + Q.RQ_WORDS * n,), SENT_WORD, dtype=torch.int64, device=ctx.device)
    d_r = rbuf[GW:GW + Q.RQ_WORDS * n]
    reads = Reads(d_b.data_ptr() if n else None, n, read_len, d_off.data_ptr() if off is not None else None)
    st = ctx.lib.kmx_reads_quality(ctx._h, C.byref(reads), ptr(d_q), phred, min_q, trim_q, k, ptr(d_w), ptr(d_m) if mask else None,
                                   ptr(d_r) if rows else None)
    assert st == OK, ctx.lib.kmx_last_error(ctx._h)
    ctx.synchronize()
    got_rows = u64(rbuf)
    assert (got_rows[:GW] == np.uint64(SENT_WORD & Q.M64)).all() and (got_rows[GW + Q.RQ_WORDS * n:] == np.uint64(SENT_WORD & Q.M64)).all()
    got_rows = got_rows[GW:GW + Q.RQ_WORDS * n].reshape(n, Q.RQ_WORDS)
    if rows:
        bad = np.nonzero((got_rows != want[1]).any(axis=1))[0]
        assert len(bad) == 0, (int(bad[0]), got_rows[bad[0]].tolist(), want[1][bad[0]].tolist())
    else:
        assert (got_rows == np.uint64(SENT_WORD & Q.M64)).all()
    # the bytes of the reads are the reference's, every other byte of the buffer is as it was
    inside = np.zeros(total, bool)
    for a, L in Q.bounds(n, read_len, off):
        inside[a:a + L] = True
    if inplace:
        got = d_b.cpu().numpy()
        expect = np.where(inside, want[0], bases)
    else:
        whole = mbuf.cpu().numpy()
        assert (whole[:GUARD + mshift] == SENT).all() and (whole[GUARD + mshift + total:] == SENT).all()
        got = whole[GUARD + mshift:GUARD + mshift + total]
        expect = np.where(inside, want[0], SENT).astype(np.uint8) if mask else np.full(total, SENT, np.uint8)
    bad = np.nonzero(got != expect)[0]
    assert len(bad) == 0, (int(bad[0]), int(got[bad[0]]), int(expect[bad[0]]))
    return got, got_rows


def test_read_lengths_and_cut_overs(ctx):
    """every length at which the wave's walk changes: within one step, the step's 256 bytes with each of the four grid phases, a second and
    a third step, 70 000 bases (274 steps with carried state); offsets[0] > 0; N and lower case; weights; k = 31"""
    rng = np.random.default_rng(11)
    lens = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 252, 253, 254, 0, 0, 509, 510, 511, 512, 513, 514, 3, 70000, 2]
    bases, quals, off = make_batch(rng, lens, first=5)
    _, rows = run(ctx, bases, quals, len(lens), 0, off, bshift=3, qshift=1, mshift=2, min_q=12, trim_q=20, k=31, weights=Q.ee_weights(33))
    assert rows[:, Q.RQ_BASES].tolist() == lens and int(rows[:, Q.RQ_LOW].sum()) > 0 and int(rows[24, Q.RQ_TRIM] >> np.uint64(32)) > 256


def test_alignments(ctx):
    """d_bases at byte offsets 0..15 crossed with d_quals at 0, 1, 3, 7, 13 (and d_masked at a third phase): one reference"""
    rng = np.random.default_rng(12)
    lens = [0, 3, 70, 1, 150, 0, 0, 257, 5, 4, 2, 101]
    bases, quals, off = make_batch(rng, lens, first=2)
    kw = dict(min_q=15, trim_q=18, k=5, weights=Q.ee_weights(33))
    want = Q.reads_quality_np(bases, quals, len(lens), 0, off, 33, kw["min_q"], kw["trim_q"], kw["k"], kw["weights"])
    for bshift in range(16):
        for qshift in (0, 1, 3, 7, 13):
            run(ctx, bases, quals, len(lens), 0, off, bshift=bshift, qshift=qshift, mshift=(bshift * 5 + qshift) % 4, want=want, **kw)
    # rows alone: the grid is then that of d_bases
    for bshift in (0, 1, 2, 3):
        run(ctx, bases, quals, len(lens), 0, off, bshift=bshift, qshift=2, want=want, mask=False, **kw)


@pytest.mark.parametrize("phred", [33, 64])
def test_extreme_quality_patterns(ctx, phred):
    rng = np.random.default_rng(13 + phred)
    lens = [150, 0, 37, 300, 64]
    bases, quals, off = make_batch(rng, lens)
    n = len(lens)
    w = rng.integers(0, 2**63, 256).astype(np.uint64) * np.uint64(2) + np.uint64(1)   # sums that wrap

    def go(q, **kw):
        return run(ctx, bases, q, n, 0, off, bshift=1, qshift=2, mshift=3, phred=phred, weights=w, **kw)[1]

    r = go(np.full_like(quals, phred + 5), min_q=6, trim_q=3, k=4)            # all bases below min_q
    assert r[:, Q.RQ_LOW].tolist() == lens and not r[:, Q.RQ_RUN].any() and not r[:, Q.RQ_WINDOWS].any()
    r = go(np.full_like(quals, phred + 5), min_q=5, trim_q=3, k=4)            # none below
    assert not r[:, Q.RQ_LOW].any()
    r = go(np.full_like(quals, phred + 20), min_q=0, trim_q=20, k=4)          # q == trim_q everywhere: V = 0
    assert not r[:, Q.RQ_TRIM].any()
    # plateaus: +4 -4 +4 0 0 +4 -4 repeated (both tie rules at once, across lanes and across the 256-byte step)
    pat = np.array([9, 1, 9, 5, 5, 9, 1], np.uint8) + np.uint8(phred)
    go(np.resize(pat, len(quals)), min_q=5, trim_q=5, k=2)
    go(np.resize(np.array([5, 5, 9, 9, 5, 5, 1, 9, 1, 9], np.uint8) + np.uint8(phred), len(quals)), min_q=2, trim_q=5, k=3)
    r = go(rng.integers(0, phred + 3, len(quals)).astype(np.uint8), min_q=1, trim_q=1, k=2)       # bytes below phred_base: q = 0
    assert int(r[:, Q.RQ_LOW].sum()) > 0
    r = go(rng.integers(0x80, 0x100, len(quals)).astype(np.uint8), min_q=60, trim_q=100, k=2)     # bytes >= 0x80
    assert int((r[0, Q.RQ_MINMAX] >> np.uint64(32))) >= 0x80 - phred
    go(rng.integers(0, 0x100, len(quals)).astype(np.uint8), min_q=255, trim_q=255, k=1)
    go(rng.integers(0, 0x100, len(quals)).astype(np.uint8), min_q=0, trim_q=0, k=1)


def test_uniform_reads_and_k(ctx):
    """uniform reads (d_offsets NULL, L not a multiple of four: every grid phase); k in {0, 1, 31, L, L + 1}"""
    rng = np.random.default_rng(14)
    n, L = 37, 101
    bases, quals, _ = make_batch(rng, [n * L], qlo=33 + 2, qhi=33 + 40)
    for k in (0, 1, 31, L, L + 1):
        r = run(ctx, bases, quals, n, L, None, bshift=5, qshift=9, mshift=1, min_q=4, trim_q=25, k=k)[1]
        assert (k == 0) == (not r[:, Q.RQ_WINDOWS].any()) or k >= L
    clean = np.full(n * L, ord("A"), np.uint8)
    r = run(ctx, clean, quals, n, L, None, min_q=0, trim_q=0, k=L)[1]
    assert r[:, Q.RQ_WINDOWS].tolist() == [1] * n
    r = run(ctx, clean, quals, n, L, None, min_q=0, trim_q=0, k=L + 1)[1]
    assert not r[:, Q.RQ_WINDOWS].any()


def test_more_reads_than_the_grid_has_waves(ctx):
    """a wave takes a second and a third read: masked bytes of the whole batch against numpy, rows of three stretches against the reference"""
    import torch

    rng = np.random.default_rng(15)
    n, L = 3 * 32768 + 11, 6
    bases, quals, _ = make_batch(rng, [n * L])
    masked, rows = ctx.reads_quality(ctx.to_device(bases), ctx.to_device(quals), n, L, min_q=20, trim_q=20, k=3)
    torch.cuda.synchronize()
    assert (masked.cpu().numpy() == np.where(quals.astype(np.int64) - 33 < 20, ord("N"), bases)).all()
    got = u64(rows)
    for lo in (0, 32768 - 20, n - 40):
        want = Q.reads_quality_np(bases[lo * L:(lo + 40) * L], quals[lo * L:(lo + 40) * L], 40, L, None, 33, 20, 20, 3)[1]
        assert (got[lo:lo + 40] == want).all()


def test_in_place_and_repeatable(ctx):
    rng = np.random.default_rng(16)
    lens = [150, 0, 1, 149, 151, 300, 2]
    bases, quals, off = make_batch(rng, lens, first=1)
    kw = dict(min_q=20, trim_q=20, k=31)
    a = run(ctx, bases, quals, len(lens), 0, off, bshift=3, qshift=6, mshift=1, **kw)
    b = run(ctx, bases, quals, len(lens), 0, off, bshift=3, qshift=6, mshift=1, **kw)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    c = run(ctx, bases, quals, len(lens), 0, off, bshift=3, qshift=6, inplace=True, **kw)
    inside = np.zeros(len(bases), bool)
    for s, L in Q.bounds(len(lens), 0, off):
        inside[s:s + L] = True
    assert (c[0][inside] == a[0][inside]).all() and c[1].tobytes() == a[1].tobytes()
    run(ctx, bases, quals, len(lens), 0, off, rows=False, **kw)


def test_argument_errors(ctx):
    import torch
    from kmers_amd._lib import Reads

    bases = ctx.to_device(np.full(64, ord("A"), np.uint8))
    quals = ctx.to_device(np.full(128, ord("I"), np.uint8))
    rows = torch.zeros(8 * 4, dtype=torch.int64, device=ctx.device)
    out = torch.zeros(64, dtype=torch.uint8, device=ctx.device)
    reads = Reads(bases.data_ptr(), 4, 16, None)
    f = ctx.lib.kmx_reads_quality

    def call(r=reads, q=quals, phred=33, min_q=0, trim_q=0, m=out, rw=rows):
        return f(ctx._h, C.byref(r) if r is not None else None, ptr(q), phred, min_q, trim_q, 0, None, ptr(m), ptr(rw))

    assert call() == OK
    assert call(phred=256) == E_ARG and call(min_q=256) == E_ARG and call(trim_q=256) == E_ARG
    assert call(q=None) == E_ARG                     # d_quals NULL with reads present
    assert call(m=None, rw=None) == E_ARG            # both outputs NULL
    assert call(m=None) == OK and call(rw=None) == OK
    assert call(r=None) == E_ARG and f(None, C.byref(reads), ptr(quals), 33, 0, 0, 0, None, ptr(out), ptr(rows)) == E_ARG
    assert call(m=bases) == OK                       # in place
    assert call(m=bases[1:]) == E_ARG                # any other overlap with the bases ...
    assert call(m=quals[60:]) == E_ARG               # ... and any with the quality bytes
    off = ctx.to_device(np.array([0, 10, 10, 30, 64], np.uint64))
    ragged = Reads(bases.data_ptr(), 4, 0, off.data_ptr())
    assert call(r=ragged) == OK and call(r=ragged, m=bases) == OK and call(r=ragged, m=bases[8:]) == E_ARG
    assert call(r=Reads(None, 0, 16, None), q=None) == OK      # no reads: a no-op
    ctx.synchronize()


def test_agrees_with_count_read_stats_on_the_masked_batch(ctx):
    """RQ_WINDOWS is RS_N_VALID of the masked reads; with solid_min = 0 every valid window is solid, so RS_SPAN (in windows) is RQ_RUN
    (in bases) wherever the run is at least k bases"""
    from kmers_amd import _lib

    rng = np.random.default_rng(17)
    lens = rng.integers(0, 260, 300).tolist() + [600]
    bases, quals, off = make_batch(rng, lens, qlo=33 + 8, qhi=33 + 41)
    n, k = len(lens), 9
    d_off = ctx.to_device(off)
    masked, rows = ctx.reads_quality(ctx.to_device(bases), ctx.to_device(quals), n, max(lens), min_q=10, k=k, offsets=d_off)
    kmers, counts = ctx.count_canonical(masked, n, max(lens), k, offsets=d_off)
    rq = u64(rows)
    for table in ((kmers, counts), (kmers[:1], counts[:1])):
        rs = u64(ctx.count_read_stats(masked, n, max(lens), k, table[0], table[1], solid_min=0, offsets=d_off))
        assert (rs[:, _lib.RS_N_VALID] == rq[:, Q.RQ_WINDOWS]).all() and int(rq[:, Q.RQ_WINDOWS].sum()) > 0
        run_len = (rq[:, Q.RQ_RUN] >> np.uint64(32)).astype(np.int64)
        has = run_len >= k
        assert has.sum() > 50
        want_span = (rq[:, Q.RQ_RUN] & np.uint64(0xFFFFFFFF)) | ((run_len - k + 1).astype(np.uint64) << np.uint64(32))
        assert (rs[has, _lib.RS_SPAN] == want_span[has]).all()
        assert not rs[~has, _lib.RS_SPAN].any()


@pytest.mark.parametrize("trim", ["mott", "run", None])
def test_reads_quality_filter(ctx, trim):
    from kmers_amd.api import expected_errors

    rng = np.random.default_rng(18)
    lens = rng.integers(0, 200, 200).tolist()
    bases, quals, off = make_batch(rng, lens, first=3, qlo=33 + 2, qhi=33 + 40)
    n = len(lens)
    d_off = ctx.to_device(off)
    b, q, rows = ctx.reads_quality_filter(ctx.to_device(bases), ctx.to_device(quals), n, max(lens), min_q=7, trim_q=15, k=5, offsets=d_off,
                                          max_ee=8.0, min_len=20, trim=trim)
    want_m, want_r = Q.reads_quality_np(bases, quals, n, 0, off, 33, 7, 15, 5, Q.ee_weights(33))
    assert (u64(rows) == want_r).all()
    assert np.allclose(expected_errors(rows).cpu().numpy(), Q.expected_errors_np(want_r), rtol=0, atol=1e-9)
    keep = Q.expected_errors_np(want_r) <= 8.0
    span = None if trim is None else want_r[:, Q.RQ_TRIM if trim == "mott" else Q.RQ_RUN]
    for batch, src in ((b, want_m), (q, quals)):
        out, o, idx = reads_np.select_np(src, n, 0, off, keep=keep, span=span, span_k=0, min_len=20)
        assert batch.n_reads == len(idx) and 0 < len(idx) < n
        assert (u64(batch.offsets) == o).all() and batch.bases.cpu().numpy().tobytes() == out.tobytes()
    assert (u64(b.offsets) == u64(q.offsets)).all() and (u64(b.index) == idx).all()
