"""Pass 2 of the bit-sliced scan (phase D on the matrix pipe, kmx_bitslice_kernel.h) at the shapes where it can break.

The single-word uniform variants (ASCII and SeqVector input) run pass 2 unguarded, as one basic block: every one of a lane's WPL window
blocks goes through the matrix instructions, a block past the last window with all-zero mask words.  The two-word k, ragged reads and
segments of long reads keep the run-time guard.  What is checked, always exactly -- {n_valid, sum_canon, xor_hash, sum_fw} against the
CPU oracle, with the hash fold on and off and with KMX_REDUCE_SUM_FW on and off:

  * every frame (5 / 7 / 8 / 10 / 11 / 13 / 16 words) at the read lengths that put W = L - k + 1 on both sides of every multiple of 32
    the frame can hold (W = 32 j: the last window block full; W = 32 j + 1: one window in it), plus the frame's longest read, for
    k in {9, 13, 21, 30, 31} -- both parities (the odd k skip the middle pair's ripple step), the fewest and the most accumulator blocks;
  * 32 * n_cu * 64 + 37 reads a case: every wave takes several tiles, and the batch ends in a partial tile;
  * the 10-word frame at k = 31 once at 256 * 3 * 4 * n_cu * 64 reads: the one case where the waves fold their fp32 accumulators
    (BS_FOLD_TILES = 256 tiles a wave).  Its oracle is exact too: the batch is 255 copies of one block of reads and one copy of
    another, and every word of the summary is a wrapping sum or an xor over reads;
  * the 10- and the 16-word frame through kmx_seqvec_canonical_reduce, the same lengths; and the launches that DO have an empty
    window block: packed reads far shorter than their frame, uniform reads behind an offsets array at a length below the bound;
  * the variants that keep the guard: k = 63 at L = 150 and L = 250, one ragged batch, one batch of 300-base reads (segments).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = (9, 13, 21, 30, 31)
# (words, shortest read, longest read) of the frames launch_bs_any picks for ASCII reads from a 16-byte aligned base
FRAMES = ((5, 0, 80), (7, 81, 112), (8, 113, 128), (10, 129, 160), (11, 161, 176), (13, 161, 208), (16, 209, 256))


def frame_of(L, k):
    """the frame a uniform batch of L-base reads is scanned in (kmx_bitslice_kernel.h, launch_bs_any)"""
    for nw, _, hi in FRAMES:
        if L <= hi and not (nw == 11 and L - k + 1 > 160):
            return nw
    raise ValueError(L)


def lengths(nw, k):
    """read lengths of frame `nw` with W on both sides of a multiple of 32, and the frame's longest read"""
    lo, hi = next((a, b) for n, a, b in FRAMES if n == nw)
    out = [L for L in range(max(lo, k + 31), hi + 1) if (L - k + 1) % 32 in (0, 1) and frame_of(L, k) == nw]
    top = max(L for L in range(lo, hi + 1) if frame_of(L, k) == nw)
    return sorted(set(out + [top]))


CASES = [(nw, k, L) for nw, _, _ in FRAMES for k in KS for L in lengths(nw, k)]
PACKED_CASES = [(nw, k, L) for nw in (10, 16) for k in KS for L in lengths(nw, k)]


def test_case_table_covers_every_frame_and_both_sides():
    """(no GPU work: the table above is what the parametrised tests below run)"""
    assert {nw for nw, _, _ in CASES} == {5, 7, 8, 10, 11, 13, 16}
    for nw, _, _ in FRAMES:
        for k in KS:
            ws = {(L - k + 1) % 32 for n, kk, L in CASES if n == nw and kk == k}
            assert ws, (nw, k)
    for nw in (5, 7, 10, 13, 16):     # (the 8- and the 11-word frame span 16 read lengths: not every k meets a multiple of 32 there)
        for k in KS:
            ws = {(L - k + 1) % 32 for n, kk, L in CASES if n == nw and kk == k}
            assert {0, 1} <= ws, (nw, k, ws)


@pytest.fixture(scope="module")
def ctx():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from kmers_amd.api import Context

    c = Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def n_cu(ctx):
    import torch

    return torch.cuda.get_device_properties(ctx.device).multi_processor_count


def _modes():
    from kmers_amd import _lib

    return [(h, f) for h in (_lib.HASH_NONE, _lib.HASH_LEX) for f in (0, _lib.REDUCE_SUM_FW)]


def _expect(o, hasher, flags):
    return (o.n_valid, o.sum_canon, o.xor_hash if hasher else 0, o.sum_fw if flags else 0)


def _got(g):
    return (g.n_valid, g.sum_canon, g.xor_hash, g.sum_fw)


def _batch(ctx, n, L, seed):
    dev = ctx.gen_reads(n * L, first_byte=seed)
    return dev, dev.cpu().numpy()


@pytest.mark.parametrize("nw,k,L", CASES, ids=[f"nw{nw}-k{k}-L{L}" for nw, k, L in CASES])
def test_uniform_frames(ctx, orc, n_cu, nw, k, L):
    n = 32 * n_cu * 64 + 37
    dev, host = _batch(ctx, n, L, 1000 * k + L)
    o = orc.canonical_reduce(host, n, L, k, hasher_k=k)
    assert o.n_valid == n * (L - k + 1)
    for hasher, flags in _modes():
        g = ctx.canonical_reduce(dev, n, L, k, hasher, k if hasher else 0, flags)
        assert _got(g) == _expect(o, hasher, flags), (hasher, flags)


def test_headline_frame_through_the_accumulator_fold(ctx, orc, n_cu):
    """k = 31, L = 150 at 256 * 3 * 4 * n_cu * 64 reads: 256 tiles a wave on average, so the waves fold their accumulators"""
    import torch

    k, L, reps = 31, 150, 256
    n = 256 * 3 * 4 * n_cu * 64
    b = n // reps
    d_a, h_a = _batch(ctx, b, L, 31)
    d_b, h_b = _batch(ctx, b, L, 32)
    o_a = orc.canonical_reduce(h_a, b, L, k, hasher_k=k)
    o_b = orc.canonical_reduce(h_b, b, L, k, hasher_k=k)
    m = (1 << 64) - 1

    class O:
        n_valid = (reps - 1) * o_a.n_valid + o_b.n_valid
        sum_canon = ((reps - 1) * o_a.sum_canon + o_b.sum_canon) & m
        xor_hash = o_a.xor_hash ^ o_b.xor_hash        # (an odd number of copies of block a)
        sum_fw = ((reps - 1) * o_a.sum_fw + o_b.sum_fw) & m

    dev = torch.empty(n * L, dtype=torch.uint8, device=ctx.device)
    rows = dev.view(reps, b * L)
    rows[: reps - 1] = d_a
    rows[reps - 1] = d_b
    for hasher, flags in _modes():
        g = ctx.canonical_reduce(dev, n, L, k, hasher, k if hasher else 0, flags)
        assert _got(g) == _expect(O, hasher, flags), (hasher, flags)


@pytest.mark.parametrize("nw,k,L", PACKED_CASES, ids=[f"nw{nw}-k{k}-L{L}" for nw, k, L in PACKED_CASES])
def test_packed_frames(ctx, orc, n_cu, nw, k, L):
    n = 32 * n_cu * 64 + 37
    dev, host = _batch(ctx, n, L, 2000 * k + L)
    o = orc.canonical_reduce(host, n, L, k, hasher_k=k)
    words = ctx.seqvec_from_bytes(dev)
    for hasher, flags in _modes():
        g = ctx.seqvec_canonical_reduce(words, n, L, k, hasher, k if hasher else 0, flags)
        assert _got(g) == _expect(o, hasher, flags), (hasher, flags)


# packed reads take the 10-word frame at three windows per lane from the shortest read on and the 16-word frame always at eight:
# (k, L) with two, one (10-word frame) and three, one (16-word frame) window blocks past the last window
@pytest.mark.parametrize("k,L", [(31, 50), (30, 93), (21, 84), (31, 170), (9, 200), (13, 161)])
def test_packed_reads_with_empty_window_blocks(ctx, orc, n_cu, k, L):
    n = 32 * n_cu * 64 + 37
    dev, host = _batch(ctx, n, L, 3000 * k + L)
    o = orc.canonical_reduce(host, n, L, k, hasher_k=k)
    words = ctx.seqvec_from_bytes(dev)
    for hasher, flags in _modes():
        g = ctx.seqvec_canonical_reduce(words, n, L, k, hasher, k if hasher else 0, flags)
        assert _got(g) == _expect(o, hasher, flags), (hasher, flags)


@pytest.mark.parametrize("k,L,bound", [(31, 100, 150), (21, 130, 160), (30, 180, 250)])
def test_gate_leaves_a_length_below_the_bound(ctx, orc, n_cu, k, L, bound):
    """reads of ONE length behind an offsets array: the device-side gate hands them to the uniform kernel laid out for `bound`, which
    scans them at the length the gate found -- fewer windows than its windows per lane were chosen for"""
    from kmers_amd import _lib

    n = 32 * n_cu * 64 + 37
    dev, host = _batch(ctx, n, L, 4000 * k + L)
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    o = orc.canonical_reduce(host, n, bound, k, hasher_k=k, offsets=offs)
    d_offs = ctx.to_device(offs)
    for hasher in (_lib.HASH_NONE, _lib.HASH_LEX):
        g = ctx.canonical_reduce(dev, n, bound, k, hasher, k if hasher else 0, 0, offsets=d_offs)
        assert _got(g) == _expect(o, hasher, 0), hasher


# ------------------------------------------------------------------ the variants that keep the guard
@pytest.mark.parametrize("L", [150, 250])
def test_two_word_k_keeps_its_results(ctx, orc, n_cu, L):
    k = 63
    n = 32 * n_cu * 64 + 37
    dev, host = _batch(ctx, n, L, 63 + L)
    o = orc.canonical_reduce2(host, n, L, k, with_hash=True)
    g = ctx.canonical_reduce2(dev, n, L, k, with_hash=True)
    assert (g.n_valid, g.sum_lo, g.sum_hi, g.xor_lo, g.xor_hi) == (o.n_valid, o.sum_lo, o.sum_hi, o.xor_lo, o.xor_hi)


def test_ragged_reads_keep_their_results(ctx, orc, n_cu):
    from kmers_amd import _lib

    k, bound = 31, 150
    n = 32 * n_cu * 64 + 37
    rng = np.random.default_rng(5)
    lens = np.where(rng.random(n) < 0.7, bound, rng.integers(36, bound + 1, n)).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    dev = ctx.gen_reads(int(offs[-1]), first_byte=7)
    o = orc.canonical_reduce(dev.cpu().numpy(), n, bound, k, hasher_k=k, offsets=offs)
    d_offs = ctx.to_device(offs)
    for hasher, flags in _modes():
        g = ctx.canonical_reduce(dev, n, bound, k, hasher, k if hasher else 0, flags, offsets=d_offs)
        assert _got(g) == _expect(o, hasher, flags), (hasher, flags)


def test_segments_of_long_reads_keep_their_results(ctx, orc, n_cu):
    k, L = 31, 300
    n = 32 * n_cu * 64 + 37
    dev, host = _batch(ctx, n, L, 300)
    o = orc.canonical_reduce(host, n, L, k, hasher_k=k)
    for hasher, flags in _modes():
        g = ctx.canonical_reduce(dev, n, L, k, hasher, k if hasher else 0, flags)
        assert _got(g) == _expect(o, hasher, flags), (hasher, flags)
