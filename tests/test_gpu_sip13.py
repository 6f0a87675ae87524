"""The *_sip13 calls on the GPU: kmx_canonical_reduce_sip13, kmx_histogram_sip13 and the three minimizer calls under std's
DefaultHasher (keys 0, 0) / RandomState (a random key pair) -- SipHash-1-3 of the word's 8 little-endian bytes (hash.rs:4-20).

Expected values: the oracle's canonical_windows (canonical words, validity) hashed by the numpy SipHash (tests/sip13_np.py, pinned
to the oracle's kmo_siphash13_u64 in test_sip13_host.py); the minimizers against a numpy restatement of the monotone deque that is
itself checked against oracle.seqvec_minimizers first.  At size the oracle cannot keep up: already-pinned device primitives
(kmx_canonical_windows, kmx_hash_words_sip13, kmx_seqvec_push_chars) are composed instead."""
import numpy as np
import pytest

from tests import sip13_np

pytestmark = pytest.mark.gpu

KEYS = [(0, 0), (0x0706050403020100, 0x0F0E0D0C0B0A0908), (0xA5C3_11F0_9B2E_7D41, 0x3C6E_F372_FE94_F82B), (2**64 - 1, 1)]


@pytest.fixture(scope="module")
def ctx():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from kmers_amd.api import Context

    c = Context()
    yield c
    c.close()


def _acgt(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()


def _dirty(host, starts, lens, rng, share):
    """N in a share of the reads (first and last base included), lower case in others"""
    n = len(lens)
    for i, r in enumerate(np.nonzero(rng.random(n) < share)[0]):
        s, ln = int(starts[r]), int(lens[r])
        if ln == 0:
            continue
        host[s + (0 if i % 3 == 0 else ln - 1 if i % 3 == 1 else int(rng.integers(0, ln)))] = ord("N")
    for r in np.nonzero(rng.random(n) < 0.05)[0]:
        s, ln = int(starts[r]), int(lens[r])
        host[s: s + ln] |= 0x20          # lower case: still bases


def _expect(orc, host, n, L, k, offsets, k0, k1):
    _, _, canon, flags = orc.canonical_windows(host, n, L, k, offsets)
    valid = (flags & 1) != 0
    return canon[valid], sip13_np.siphash13(canon[valid], k0, k1)


def _check_reduce(ctx, orc, dev, host, n, L, k, offsets_host, offsets_dev, flags_list=(0, 1)):
    for k0, k1 in KEYS:
        canon, h = _expect(orc, host, n, L, k, offsets_host, k0, k1)
        want_x = int(np.bitwise_xor.reduce(h)) if len(h) else 0
        for fl in flags_list:
            g = ctx.canonical_reduce_sip13(dev, n, L, k, k0, k1, flags=fl, offsets=offsets_dev)
            lex = ctx.canonical_reduce(dev, n, L, k, 0, 0, flags=fl, offsets=offsets_dev)
            assert g.xor_hash == want_x, (k, L, k0, k1, fl)
            assert (g.n_valid, g.sum_canon, g.sum_fw) == (lex.n_valid, lex.sum_canon, lex.sum_fw)
            assert g.n_valid == len(canon)
    # swapping the keys changes the hash (k >= 9: enough distinct words that the xor does not cancel)
    k0, k1 = KEYS[1]
    _, h = _expect(orc, host, n, L, k, offsets_host, k1, k0)
    b = ctx.canonical_reduce_sip13(dev, n, L, k, k1, k0, offsets=offsets_dev)
    assert b.xor_hash == (int(np.bitwise_xor.reduce(h)) if len(h) else 0)
    if k >= 9 and len(h) > 100:
        assert b.xor_hash != ctx.canonical_reduce_sip13(dev, n, L, k, k0, k1, offsets=offsets_dev).xor_hash


# ---------------------------------------------------------------- reduce
@pytest.mark.parametrize("k", [1, 2, 9, 12, 13, 16, 17, 21, 31])
@pytest.mark.parametrize("L", [31, 150, 160, 161, 256, 300, 1000])
def test_reduce_uniform(ctx, orc, k, L):
    rng = np.random.default_rng(k * 1000 + L)
    n = max(64 * 3 + 5, 30000 // L)
    host = _acgt(rng, n * L)
    _dirty(host, np.arange(n) * L, np.full(n, L), rng, 0.02 if L != 300 else 0.1)
    _check_reduce(ctx, orc, ctx.to_device(host), host, n, L, k, None, None)


@pytest.mark.parametrize("k", [2, 13, 31])
def test_reduce_read_of_k_bases_and_odd_address(ctx, orc, k):
    import torch

    rng = np.random.default_rng(k)
    for L, share in ((k, 0.005), (150, 0.5)):
        n = 64 * 2 + 9
        host = _acgt(rng, n * L)
        _dirty(host, np.arange(n) * L, np.full(n, L), rng, share)
        big = torch.empty(n * L + 3, dtype=torch.uint8, device="cuda")
        big[3:] = torch.from_numpy(host).cuda()
        _check_reduce(ctx, orc, big[3:], host, n, L, k, None, None, flags_list=(0,))


@pytest.mark.parametrize("k", [1, 9, 17, 31])
@pytest.mark.parametrize("bound", [0, 150, 256])
def test_reduce_ragged(ctx, orc, k, bound):
    import torch

    rng = np.random.default_rng(k * 7 + bound)
    n = 64 * 4 + 11
    hi = bound if bound else 300
    lens = rng.integers(0, hi + 1, n).astype(np.int64)
    lens[:5] = [0, 1, k - 1 if k > 1 else 0, k, hi]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    host = _acgt(rng, int(offs[-1]))
    _dirty(host, offs[:-1], lens, rng, 0.1)
    _check_reduce(ctx, orc, ctx.to_device(host), host, n, bound, k, offs, ctx.to_device(offs))
    # a misaligned d_bases (the lane-per-read kernel)
    big = torch.empty(int(offs[-1]) + 5, dtype=torch.uint8, device="cuda")
    big[5:] = torch.from_numpy(host).cuda()
    _check_reduce(ctx, orc, big[5:], host, n, bound, k, offs, ctx.to_device(offs), flags_list=(0,))


def test_reduce_empty_batch_is_zero(ctx):
    import torch

    dev = torch.zeros(16, dtype=torch.uint8, device="cuda")
    g = ctx.canonical_reduce_sip13(dev, 0, 150, 31, 1, 2, flags=1)
    assert (g.n_valid, g.sum_canon, g.xor_hash, g.sum_fw) == (0, 0, 0, 0)


# ---------------------------------------------------------------- histogram
@pytest.mark.parametrize("b", [0, 10, 14, 15, 20, 22, 23])
@pytest.mark.parametrize("ragged,share", [(False, 0.0), (False, 0.02), (True, 0.0), (True, 0.02)])
def test_histogram(ctx, orc, b, ragged, share):
    import torch

    k = 31 if b % 2 == 0 else 21
    rng = np.random.default_rng(b * 10 + int(ragged))
    n = 64 * 80 + 13
    if ragged:
        lens = rng.integers(0, 257, n).astype(np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        L = 256
    else:
        L = 150
        lens = np.full(n, L)
        offs = None
    starts = offs[:-1] if ragged else np.arange(n) * L
    host = _acgt(rng, int(lens.sum()))
    _dirty(host, starts, lens, rng, share)
    dev = ctx.to_device(host)
    d_offs = ctx.to_device(offs) if ragged else None
    for k0, k1 in KEYS[1:3]:
        _, h = _expect(orc, host, n, L, k, offs, k0, k1)
        want = np.bincount(sip13_np.bucket_of(h, b), minlength=1 << b).astype(np.int64)
        base = torch.arange(1 << b, dtype=torch.int64, device="cuda") % 7      # the counts accumulate
        got = ctx.histogram_sip13(dev, n, L, k, b, k0, k1, offsets=d_offs, counts=base.clone())
        assert ((got - base).cpu().numpy() == want).all(), (b, ragged, share, k0)


# ---------------------------------------------------------------- minimizers
def _mm_numpy(host_codes_2d, k, w, k0, k1):
    lm = sip13_np.lmers(host_codes_2d, w)
    return sip13_np.sliding_minimizers(lm, sip13_np.siphash13(lm.ravel(), k0, k1).reshape(lm.shape), k, w)


@pytest.mark.parametrize("k,w", [(31, 15), (21, 11), (31, 1), (31, 31), (20, 12), (31, 29), (32, 32)])
def test_numpy_deque_restatement_matches_the_oracle(orc, k, w):
    """identity hash: the numpy restatement equals the oracle's monotone deque (the tie rule included: two-letter reads)"""
    rng = np.random.default_rng(k + w)
    n, L = 40, 150
    host = _acgt(rng, n * L)
    host[: 10 * L] = np.frombuffer(b"ACAC", np.uint8)[rng.integers(0, 2, 10 * L) * 2]
    lm = sip13_np.lmers(sip13_np.codes_of(host).reshape(n, L), w)
    words, pos = sip13_np.sliding_minimizers(lm, lm, k, w)
    ow, op = orc.seqvec_minimizers(orc.SeqVector(host.tobytes()), n, L, k, w, 0)
    assert (words.ravel() == ow).all() and (pos.ravel() == op).all()


def _special_reads(rng, n, L):
    host = _acgt(rng, n * L)
    host[:L] = ord("A")                                               # poly-A: every l-mer hash equal
    host[L: 2 * L] = np.frombuffer((b"ACG" * L)[:L], np.uint8)        # tandem repeat
    host[2 * L: 3 * L] = np.frombuffer((b"AC" * L)[:L], np.uint8)
    host[3 * L: 4 * L] |= 0x20                                        # lower case
    return host


@pytest.mark.parametrize("k,w", [(31, 15), (21, 11), (31, 1), (31, 31), (20, 12), (31, 29)])
@pytest.mark.parametrize("L", [150, 256, 1000])
def test_minimizers_uniform_and_seqvec(ctx, k, w, L):
    rng = np.random.default_rng(k * 100 + w + L)
    n = max(70, 30000 // L)
    host = _special_reads(rng, n, L)
    for k0, k1 in (KEYS[0], KEYS[2]):
        ow, op = _mm_numpy(sip13_np.codes_of(host).reshape(n, L), k, w, k0, k1)
        mw, mp = ctx.minimizers_sip13(ctx.to_device(host), n, L, k, w, k0, k1)
        assert (mw.cpu().numpy().view(np.uint64) == ow.ravel()).all(), (k, w, L, k0)
        assert (mp.cpu().numpy().view(np.uint32) == op.ravel()).all()
        sv = ctx.seqvec_from_bytes(ctx.to_device(host))
        sw, sp = ctx.seqvec_minimizers_sip13(sv, n, L, k, w, k0, k1)
        assert (sw.cpu().numpy().view(np.uint64) == ow.ravel()).all()
        assert (sp.cpu().numpy().view(np.uint32) == op.ravel()).all()


@pytest.mark.parametrize("k,w", [(31, 15), (21, 11), (20, 12)])
def test_minimizers_ragged(ctx, k, w):
    rng = np.random.default_rng(k * 3 + w)
    n = 300
    lens = rng.integers(0, 600, n).astype(np.int64)
    lens[:4] = [0, k - 1, k, 256]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    wins = np.concatenate([[0], np.cumsum(np.maximum(lens - k + 1, 0))]).astype(np.uint64)
    host = _acgt(rng, int(offs[-1]))
    k0, k1 = KEYS[1]
    ow, op = [], []
    for r in range(n):
        ln = int(lens[r])
        if ln < k:
            continue
        a, b = _mm_numpy(sip13_np.codes_of(host[int(offs[r]): int(offs[r + 1])]).reshape(1, ln), k, w, k0, k1)
        ow.append(a.ravel())
        op.append(b.ravel())
    mw, mp = ctx.minimizers_sip13(ctx.to_device(host), n, 600, k, w, k0, k1, offsets=ctx.to_device(offs), win_offsets=ctx.to_device(wins))
    assert (mw.cpu().numpy().view(np.uint64) == np.concatenate(ow)).all()
    assert (mp.cpu().numpy().view(np.uint32) == np.concatenate(op)).all()


@pytest.mark.parametrize("k,w", [(257, 15), (300, 32), (300, 1)])
def test_minimizers_k_above_a_piece(ctx, k, w):
    """k above 256 bases (no piece of the tiled kernel holds a k-mer): the lane-per-k-mer kernel, uniform, SeqVector and ragged reads"""
    rng = np.random.default_rng(k + w)
    k0, k1 = KEYS[2]
    for L, n in ((k, 9), (300, 7), (1000, 5)):
        if L < k:
            continue
        host = _acgt(rng, n * L)
        host[:L] = ord("A")                                            # poly-A: equal hashes, the leftmost wins
        ow, op = _mm_numpy(sip13_np.codes_of(host).reshape(n, L), k, w, k0, k1)
        mw, mp = ctx.minimizers_sip13(ctx.to_device(host), n, L, k, w, k0, k1)
        assert (mw.cpu().numpy().view(np.uint64) == ow.ravel()).all(), (k, w, L)
        assert (mp.cpu().numpy().view(np.uint32) == op.ravel()).all()
        sw, sp = ctx.seqvec_minimizers_sip13(ctx.seqvec_from_bytes(ctx.to_device(host)), n, L, k, w, k0, k1)
        assert (sw.cpu().numpy().view(np.uint64) == ow.ravel()).all()
        assert (sp.cpu().numpy().view(np.uint32) == op.ravel()).all()
    lens = np.array([0, k - 1, k, 400, 1000, 299], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    wins = np.concatenate([[0], np.cumsum(np.maximum(lens - k + 1, 0))]).astype(np.uint64)
    host = _acgt(rng, int(offs[-1]))
    ow, op = [], []
    for r in range(len(lens)):
        if lens[r] >= k:
            a, b = _mm_numpy(sip13_np.codes_of(host[int(offs[r]): int(offs[r + 1])]).reshape(1, -1), k, w, k0, k1)
            ow.append(a.ravel())
            op.append(b.ravel())
    mw, mp = ctx.minimizers_sip13(ctx.to_device(host), len(lens), 0, k, w, k0, k1, offsets=ctx.to_device(offs), win_offsets=ctx.to_device(wins))
    assert (mw.cpu().numpy().view(np.uint64) == np.concatenate(ow)).all()
    assert (mp.cpu().numpy().view(np.uint32) == np.concatenate(op)).all()


def test_minimizers_one_short_read(ctx):
    """a single read of 12 bases (a batch shorter than the 20-byte loads of the Lex kernel's stand-in source)"""
    host = np.frombuffer(b"ACGTTGCAACGG", np.uint8).copy()
    for k, w in ((12, 5), (10, 3)):
        ow, op = _mm_numpy(sip13_np.codes_of(host).reshape(1, 12), k, w, *KEYS[1])
        mw, mp = ctx.minimizers_sip13(ctx.to_device(host), 1, 12, k, w, *KEYS[1])
        assert (mw.cpu().numpy().view(np.uint64) == ow.ravel()).all()
        assert (mp.cpu().numpy().view(np.uint32) == op.ravel()).all()


def test_minimizers_invalid_byte_is_reported(ctx):
    from kmers_amd import _lib
    from kmers_amd.api import KmxError

    rng = np.random.default_rng(5)
    n, L = 100, 150
    host = _acgt(rng, n * L)
    host[57 * L + 149] = ord("N")
    host[80 * L] = ord("N")
    with pytest.raises(KmxError) as ei:
        ctx.minimizers_sip13(ctx.to_device(host), n, L, 31, 15, 3, 4)
    assert ei.value.status == _lib.E_INVALID_BASE and ei.value.first_bad == 57
    mw, _ = ctx.minimizers_sip13(ctx.to_device(host), n, L, 31, 15, 3, 4, check=False)
    assert mw.numel() == n * 120


@pytest.mark.parametrize("k,w", [(31, 15), (21, 11), (32, 32), (31, 1), (31, 31), (20, 12), (31, 29)])
def test_minimizer_words(ctx, orc, k, w):
    """Kmer::minimizer_word with a SipHash state; the kmer.rs:560-580 property: the chosen l-mer's hash is <= every other l-mer's
    hash of the k-mer, and the l-mer at the offset is the minimizer"""
    import torch

    rng = np.random.default_rng(k * 40 + w)
    words = rng.integers(0, 2**63, 5000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 5000, dtype=np.uint64)
    if k < 32:
        words &= np.uint64((1 << (2 * k)) - 1)
    words[:3] = [0, 0x5555555555555555 & ((1 << (2 * k)) - 1 if k < 32 else 2**64 - 1), 0]   # all-A and repeats: equal hashes
    mask = np.uint64((1 << (2 * w)) - 1 if w < 32 else 2**64 - 1)
    for k0, k1 in KEYS:
        d = torch.from_numpy(words.view(np.int64)).cuda()
        mm, off = ctx.minimizer_words_sip13(d, k, w, k0, k1)
        mm, off = mm.cpu().numpy().view(np.uint64), off.cpu().numpy()
        subs = np.stack([(words >> np.uint64(2 * p)) & mask for p in range(k - w + 1)], axis=1)
        hs = sip13_np.siphash13(subs.ravel(), k0, k1).reshape(subs.shape)
        want_off = np.argmin(hs, axis=1)
        assert (off == want_off).all()
        assert (mm == subs[np.arange(len(words)), want_off]).all()
        assert (hs[np.arange(len(words)), off] <= hs.min(axis=1)).all()


# ---------------------------------------------------------------- at size: composed from already-pinned device primitives
def test_reduce_and_histogram_at_size(ctx):
    import torch

    n, L, k = 10_000_000, 150, 31
    k0, k1 = KEYS[2]
    bases = ctx.gen_reads(n * L, seed=77)
    rng = np.random.default_rng(77)
    dirty = rng.choice(n, n // 50, replace=False)
    pos = rng.integers(0, L, len(dirty))
    idx = torch.from_numpy((dirty * L + pos).astype(np.int64)).cuda()
    bases[idx] = ord("N")
    g = ctx.canonical_reduce_sip13(bases, n, L, k, k0, k1)
    hist = ctx.histogram_sip13(bases, n, L, k, 20, k0, k1)
    want_x = 0
    want_h = torch.zeros(1 << 20, dtype=torch.int64, device="cuda")
    n_valid = 0
    chunk = 100_000
    for a in range(0, n, chunk):
        outs = ctx.canonical_windows(bases[a * L:(a + chunk) * L], chunk, L, k, want=("canon", "flags"))
        canon = outs["canon"][(outs["flags"] & 1) != 0]
        h = ctx.hash_words_sip13(canon, k0, k1)
        n_valid += canon.numel()
        hv = h.cpu().numpy().view(np.uint64)
        want_x ^= int(np.bitwise_xor.reduce(hv)) if len(hv) else 0
        want_h += torch.bincount(torch.from_numpy(sip13_np.bucket_of(hv, 20)).cuda(), minlength=1 << 20)
    assert g.n_valid == n_valid
    assert g.xor_hash == want_x
    assert torch.equal(hist, want_h)


def test_minimizers_at_size(ctx):
    n, L, k, w = 10_000_000, 150, 31, 15
    k0, k1 = KEYS[1]
    bases = ctx.gen_reads(n * L, seed=5)
    mw, mp = ctx.minimizers_sip13(bases, n, L, k, w, k0, k1)
    sv = ctx.seqvec_from_bytes(bases)
    sw, sp = ctx.seqvec_minimizers_sip13(sv, n, L, k, w, k0, k1)
    import torch

    assert torch.equal(mw, sw) and torch.equal(mp, sp)
    rng = np.random.default_rng(1)
    sample = np.concatenate([rng.choice(n, 1999, replace=False), [n - 1]])
    host = bases.cpu().numpy()
    W = L - k + 1
    mwh, mph = mw.cpu().numpy().view(np.uint64), mp.cpu().numpy().view(np.uint32)
    codes = np.stack([sip13_np.codes_of(host[r * L:(r + 1) * L]) for r in sample])
    ow, op = _mm_numpy(codes, k, w, k0, k1)
    for i, r in enumerate(sample):
        assert (mwh[r * W:(r + 1) * W] == ow[i]).all() and (mph[r * W:(r + 1) * W] == op[i]).all(), r
