"""Coloured tables on the GPU: kmx_count_color_matrix (kmx_count_color.hip) and the colour build of kmers_amd.api
(count_color_add(2) / count_color_build(2): kmx_count_setop(2) on filled masks).

Every comparison is u64 equality of the whole output -- guard words around it included, poison in it before the call -- against
tests/color_np.py (pinned on strings and against a second implementation in tests/test_color_np.py; sizes the plain loop is too slow for
go through its numpy form, pinned there against the loop).  The sizes: nothing, one key, one step of a wave less one / exactly / plus
one, more than a block's first sweep, and 300 000 -- more than one sweep of the grid of a 256-CU device (1024 blocks of 256 keys).
n_colors on both sides of every instantiation bound (8 / 16 / 32 / 64).  Masks carry bits at or above n_colors throughout."""
import ctypes as C

import numpy as np
import pytest

from tests.color_np import color_dict, color_matrix, color_matrix_fast
from tests.correct_np import count_kmers, revcomp_bytes, table_arrays
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import random_reads, u64

pytestmark = pytest.mark.gpu

POISON = -0x5A5A5A5A5A5A5A5B
GUARD = 16
SIZES = (0, 1, 63, 64, 65, 4097, 300_000)
COLORS = (1, 2, 7, 8, 9, 32, 33, 63, 64)


def _masks(rng, n, pattern):
    if pattern == "random":
        return rng.integers(0, 2**64, n, dtype=np.uint64)
    if pattern == "sparse":       # one or two bits, anywhere in 0 .. 63: under a small n_colors most entries have no colour left
        m = np.uint64(1) << rng.integers(0, 64, n, dtype=np.uint64)
        two = rng.random(n) < 0.5
        m[two] |= np.uint64(1) << rng.integers(0, 64, int(two.sum()), dtype=np.uint64)
        return m
    if pattern == "ones":
        return np.full(n, 2**64 - 1, np.uint64)
    assert pattern == "bit63"
    return rng.integers(0, 2**64, n, dtype=np.uint64) | np.uint64(1 << 63)


def _call(ctx, d_masks, n, n_colors, want_spectrum=True, bufs=None):
    """-> (status, whole matrix buffer, whole spectrum buffer or None), the outputs inside GUARD words of poison"""
    import torch

    from kmers_amd.api import _ptr

    nc = max(min(n_colors, 64), 1)
    mat, spec = bufs or (torch.full((2 * GUARD + nc * nc,), POISON, dtype=torch.int64, device=ctx.device),
                         torch.full((2 * GUARD + nc + 1,), POISON, dtype=torch.int64, device=ctx.device))
    st = ctx.lib.kmx_count_color_matrix(ctx._h, _ptr(d_masks) if n else None, n, n_colors, _ptr(mat[GUARD:]),
                                        _ptr(spec[GUARD:]) if want_spectrum else None)
    ctx.synchronize()
    return st, mat, spec


def _check(ctx, masks, n_colors, want_spectrum=True, bufs=None):
    from kmers_amd import _lib

    n = len(masks)
    matrix, spectrum = (color_matrix if n <= 5000 and n_colors <= 9 else color_matrix_fast)(masks, n_colors)
    d = ctx.to_device(masks) if n else None
    st, mat, spec = _call(ctx, d, n, n_colors, want_spectrum, bufs)
    assert st == _lib.OK
    want = np.full(len(mat), POISON, np.int64).view(np.uint64)
    want[GUARD:GUARD + n_colors * n_colors] = matrix.reshape(-1)
    assert (u64(mat) == want).all(), (n, n_colors, np.nonzero(u64(mat) != want)[0][:8] - GUARD)
    wants = np.full(len(spec), POISON, np.int64).view(np.uint64)
    if want_spectrum:
        wants[GUARD:GUARD + n_colors + 1] = spectrum
    assert (u64(spec) == wants).all(), (n, n_colors, u64(spec)[GUARD:GUARD + n_colors + 1], spectrum)
    return mat, spec


# ---------------------------------------------------------------- the matrix and the spectrum
@pytest.mark.parametrize("n_colors", COLORS)
def test_matrix_sizes_and_patterns(ctx, n_colors):
    import torch

    assert SIZES[-1] > 256 * 4 * torch.cuda.get_device_properties(ctx.device).multi_processor_count   # more than one sweep of the grid
    rng = np.random.default_rng(9000 + n_colors)
    for n in SIZES:
        for pattern in ("random", "sparse", "ones", "bit63") if n < 100_000 else ("random", "ones"):
            masks = _masks(rng, n, pattern)
            _check(ctx, masks, n_colors)
            if n >= 4097 and n_colors < 64 and pattern != "ones":
                # the test's own input: bits at or above n_colors are there, and sparse masks leave entries without a colour below it
                assert (masks >> np.uint64(n_colors)).any()
                assert pattern != "sparse" or ((masks & np.uint64((1 << n_colors) - 1)) == 0).any()


def test_bits_above_n_colors_are_ignored(ctx):
    """the same low bits under different high bits give the same bytes; entries with high bits only land in the spectrum's bin 0"""
    rng = np.random.default_rng(9050)
    n, nc = 5000, 7
    low = rng.integers(0, 1 << nc, n, dtype=np.uint64)
    low[::5] = 0
    high = rng.integers(0, 2**64, n, dtype=np.uint64) & ~np.uint64((1 << nc) - 1)
    a = _check(ctx, low, nc)
    b = _check(ctx, low | high, nc)
    assert u64(a[0]).tobytes() == u64(b[0]).tobytes() and u64(a[1]).tobytes() == u64(b[1]).tobytes()
    assert int(u64(b[1])[GUARD]) == int((low == 0).sum()) and ((low | high)[::5] != 0).all()


@pytest.mark.parametrize("n_colors", (3, 33, 64))
def test_outputs_are_overwritten_spectrum_may_be_null_and_calls_agree(ctx, n_colors):
    rng = np.random.default_rng(9100 + n_colors)
    first = _check(ctx, _masks(rng, 20_000, "random"), n_colors)
    masks = _masks(rng, 7000, "sparse")
    again = _check(ctx, masks, n_colors, bufs=first)              # into the buffers the first call filled: not accumulated
    one = (u64(again[0]).tobytes(), u64(again[1]).tobytes())
    _check(ctx, np.zeros(0, np.uint64), n_colors, bufs=first)      # n == 0 overwrites with zeros
    fresh = _check(ctx, masks, n_colors)
    assert (u64(fresh[0]).tobytes(), u64(fresh[1]).tobytes()) == one
    _check(ctx, masks, n_colors, want_spectrum=False)              # d_spectrum NULL: its buffer stays poison, the matrix is the same


def test_argument_errors(ctx):
    import torch

    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    d = ctx.to_device(np.arange(100, dtype=np.uint64))
    for nc in (0, 65, 2**31):
        st, mat, spec = _call(ctx, d, 100, nc)
        assert st == _lib.E_ARG and (mat == POISON).all() and (spec == POISON).all()
    out = torch.zeros(64 * 64, dtype=torch.int64, device=ctx.device)
    f = ctx.lib.kmx_count_color_matrix
    assert f(ctx._h, None, 100, 8, _ptr(out), None) == _lib.E_ARG            # n > 0 without masks
    assert f(ctx._h, _ptr(d), 100, 8, None, None) == _lib.E_ARG              # no matrix
    assert f(ctx._h, _ptr(d), 2**40 + 1, 8, _ptr(out), None) == _lib.E_ARG
    assert f(None, _ptr(d), 100, 8, _ptr(out), None) == _lib.E_ARG
    assert f(ctx._h, None, 0, 8, _ptr(out), None) == _lib.OK                 # an empty table: zeros
    ctx.synchronize()


def test_api_color_matrix(ctx):
    """Context.count_color_matrix -> ColorMatrix on device tensors: shared, spectrum, sizes and the two measures"""
    import torch

    rng = np.random.default_rng(9150)
    nc = 5
    masks = rng.integers(0, 1 << nc, 3000, dtype=np.uint64)
    masks[:200] &= np.uint64(0b01111)                               # (colour 4 smaller than the rest)
    matrix, spectrum = color_matrix(masks, nc)
    m = ctx.count_color_matrix(ctx.to_device(masks), nc)
    assert (u64(m.shared) == matrix).all() and (u64(m.spectrum) == spectrum).all() and (u64(m.sizes) == np.diagonal(matrix)).all()
    assert ctx.count_color_matrix(ctx.to_device(masks), nc, spectrum=False).spectrum is None
    mf = matrix.astype(np.float64)
    sz = np.diagonal(mf)
    j, c = m.jaccard(), m.containment()
    assert j.is_cuda and j.dtype == torch.float64
    assert (j.cpu().numpy() == mf / (sz[:, None] + sz[None, :] - mf)).all() and (c.cpu().numpy() == mf / sz[:, None]).all()


# ---------------------------------------------------------------- the colour build
def _sample_tables(rng, k, n_samples=5, size=1200):
    """sample tables cut from overlapping stretches of one random genome, either strand"""
    genome = random_reads(rng, size)
    out = []
    for i in range(n_samples):
        a = int(rng.integers(0, size // 2))
        s = genome[a:a + int(rng.integers(size // 6, size // 2))]
        out.append(count_kmers(revcomp_bytes(s) if i % 2 else s, 1, len(s), k))
    return out


def _dev(ctx, table, k):
    tk, tc = table_arrays(table, k)
    if len(tk) == 0:
        import torch

        return torch.zeros((0, 2) if k > 31 else (0,), dtype=torch.int64, device=ctx.device), torch.zeros(0, dtype=torch.int64, device=ctx.device)
    return ctx.to_device(tk), ctx.to_device(tc)


def _same_table(got, want, k):
    tk, tm = table_arrays(want, k)
    assert got.kmers.shape == tk.shape, (got.kmers.shape, tk.shape)
    assert (u64(got.kmers) == tk).all() and (u64(got.colors) == tm).all()


@pytest.mark.parametrize("k", (15, 31, 47))
def test_color_build(ctx, k):
    rng = np.random.default_rng(9200 + k)
    samples = _sample_tables(rng, k)
    want = color_dict(samples)
    assert len({m for m in want.values()}) > 5 and any(bin(m).count("1") >= 3 for m in want.values())   # the stretches do overlap
    build = ctx.count_color_build if k <= 31 else ctx.count_color_build2
    add = ctx.count_color_add if k <= 31 else ctx.count_color_add2
    got = build([_dev(ctx, s, k) for s in samples], k=k)
    assert got.n_colors == 5 and got.k == k
    _same_table(got, want, k)
    # the matrix of what was built: the samples' sizes and what they share
    m = ctx.count_color_matrix(got.colors, got.n_colors)
    assert (u64(m.shared) == color_matrix(want.values(), 5)[0]).all()
    assert u64(m.sizes).tolist() == [len(s) for s in samples]
    # adding to None; the next free colour by default; colour 63, the sign bit of the int64 that holds the mask
    one = add(None, _dev(ctx, samples[0], k)[0])
    assert one.n_colors == 1
    _same_table(one, color_dict(samples[:1]), k)
    top = add(got, _dev(ctx, samples[1], k)[0], color=63)
    assert top.n_colors == 64 and top.k == k
    want63 = dict(want)
    for key in samples[1]:
        want63[key] = want63.get(key, 0) | (1 << 63)
    _same_table(top, want63, k)
    # an empty sample takes its colour and changes nothing else; an empty table takes a sample
    e = add(got, _dev(ctx, {}, k)[0])
    assert e.n_colors == 6
    _same_table(e, want, k)
    first = add(add(None, _dev(ctx, {}, k)[0]), _dev(ctx, samples[2], k)[0])
    assert first.n_colors == 2
    _same_table(first, {key: 2 for key in samples[2]}, k)
    # a colour that may already be set, and one past the last
    for bad in (0, 4, 64):
        with pytest.raises(ValueError):
            add(got, _dev(ctx, samples[0], k)[0], color=bad)
    with pytest.raises(ValueError):
        add(top, _dev(ctx, samples[0], k)[0])                        # (the next free colour of a table of 64 is none)
