"""The distinct-key estimator on the GPU (kmx_hll_*, Context.hll_*, count_solid(log2_blocks=None); kmx_hll.hip).

Registers are compared byte for byte with the host model tests/hll_np.py (pinned on the CPU by tests/test_hll_np.py); estimates are
compared only through the bins -- the device never computes one.  The keys the model is fed for the reads forms are the canon / flags
of kmx_canonical_windows(2), which the oracle pins elsewhere.  Shapes are the smallest at which the kernels can go wrong: both
routes of the add (block-private LDS registers up to log2_regs = 14 once a block has a key per dword it flushes, global
compare-and-swap otherwise), both sides of either cut, sixteen registers in four dwords under every lane, placed keys of every rank,
more keys than one grid sweep, a second stream.  An allowed estimate error is hll_np.tolerance(p) = 4 * 1.04 / sqrt(2^p)."""
import ctypes as C

import numpy as np
import pytest

from kmers_amd import _lib
from tests import hll_np as hl
from tests import sketch_np as sk
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import random_reads, u64
from tests.test_gpu_sketch import _read_cases, _windows

pytestmark = pytest.mark.gpu


def _regs(h):
    return h.regs.cpu().numpy()


def _keys(rng, n, words):
    a = rng.integers(0, 2**64, (n, words), dtype=np.uint64)
    return a[:, 0] if words == 1 else a


def _dev(ctx, a):
    return ctx.to_device(np.ascontiguousarray(a))


def _add_words(ctx, h, keys):
    f = ctx.hll_add_words if keys.ndim == 1 else ctx.hll_add_words2
    return f(h, _dev(ctx, keys))


def _sweep_blocks(ctx, n):
    import torch

    n_cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    return min(-(-n // 256), n_cu * _lib.SKETCH_SWEEP_LANES_PER_CU // 256)


def _block_private(ctx, n, p):
    """the route kmx_hll.hip takes for n keys (hll_add_block_private)"""
    return p <= _lib.HLL_LDS_MAX_LOG2_REGS and n >= _sweep_blocks(ctx, n) * ((1 << p) >> 2) * _lib.HLL_LDS_KEYS_PER_DWORD


# ---------------------------------------------------------------- add_words: both routes, both sides of the cuts
@pytest.mark.parametrize("words", (1, 2))
@pytest.mark.parametrize("p,n,private", ((4, 50_000, True), (4, 3, False), (9, 50_000, True), (9, 100, False), (14, 100, False),
                                         (14, 50_000, False), (15, 50_000, False), (18, 50_000, False)))
def test_add_words_matches_the_model(ctx, words, p, n, private):
    assert _block_private(ctx, n, p) == private
    rng = np.random.default_rng(100 * p + words + n)
    keys = _keys(rng, n, words)
    keys[1::7] = keys[0]                                    # one key many times among them
    h = _add_words(ctx, ctx.hll_new(p, seed=11), keys)
    exp = hl.registers(keys, p, seed=11)
    assert (_regs(h) == exp).all()
    if (p, n) == (4, 50_000):
        assert exp.min() >= 8                               # every byte of the four dwords raised many times
    more = _keys(rng, n, words)                             # accumulation: other keys on top, then the first again
    _add_words(ctx, h, more)
    exp = hl.registers(more, p, seed=11, into=exp)
    assert (_regs(h) == exp).all()
    _add_words(ctx, h, keys)
    assert (_regs(h) == exp).all()
    assert (u64(h.histogram()) == hl.bins(exp)).all()


@pytest.mark.parametrize("words", (1, 2))
def test_both_routes_at_the_lds_cut(ctx, words):
    """log2_regs = 14 on either side of the keys-per-block cut: the same keys' head through the global route, all of them through the
    block-private one, and one route on top of the other."""
    p = _lib.HLL_LDS_MAX_LOG2_REGS
    cap = _sweep_blocks(ctx, 1 << 40)
    n = cap * ((1 << p) >> 2) * _lib.HLL_LDS_KEYS_PER_DWORD + 77          # 4.2e6 on 256 compute units
    below = n - 78
    assert _block_private(ctx, n, p) and not _block_private(ctx, below, p) and not _block_private(ctx, 300_000, p)
    rng = np.random.default_rng(14 + words)
    keys = _keys(rng, n, words)
    d_keys = _dev(ctx, keys)
    add = ctx.hll_add_words if words == 1 else ctx.hll_add_words2
    exp = hl.registers(keys, p, seed=2)
    a = add(ctx.hll_new(p, seed=2), d_keys)
    assert (_regs(a) == exp).all()
    exp_below = hl.registers(keys[:below], p, seed=2)
    b = add(ctx.hll_new(p, seed=2), d_keys.view(-1)[:below * words])
    assert (_regs(b) == exp_below).all()
    add(b, d_keys)                                                        # the block-private route into registers the global one filled
    assert (_regs(b) == exp).all()
    est = hl.estimate(u64(a.histogram()), p)
    assert abs(est - n) / n <= hl.tolerance(p)                            # (random 64-bit keys: all distinct)
    assert a.estimate() == est


# ---------------------------------------------------------------- placed keys
@pytest.mark.parametrize("p", (4, 14))
def test_placed_keys_every_register_and_every_rank(ctx, p):
    q, seed = 64 - p, 5
    ones = (np.arange(1 << p, dtype=np.uint64) << np.uint64(q)) | np.uint64(1 << (q - 1))
    h = _add_words(ctx, ctx.hll_new(p, seed=seed), hl.keys_for_hashes(ones, seed))
    assert (_regs(h) == 1).all()                                          # one key per register, rank 1
    # every rank up to 65 - p, w == 0 included, in registers 3 (all of them) and r mod 2^p (one each)
    ranks = list(range(1, q + 1))
    hs = np.array([(3 << q) | (1 << (q - r)) for r in ranks] + [3 << q] +
                  [((r % (1 << p)) << q) | (1 << (q - r)) for r in ranks] + [(7 % (1 << p)) << q], np.uint64)
    keys = hl.keys_for_hashes(hs, seed)
    exp = hl.registers(np.concatenate([hl.keys_for_hashes(ones, seed), keys]), p, seed=seed)
    assert exp[3] == 65 - p == exp.max() and exp[7] == 65 - p
    _add_words(ctx, h, keys)
    assert (_regs(h) == exp).all()
    fresh = _add_words(ctx, ctx.hll_new(p, seed=seed), keys[::-1])        # the same keys in reverse order into a fresh array
    _add_words(ctx, fresh, hl.keys_for_hashes(ones, seed)[::-1])
    assert (_regs(fresh) == exp).all()
    one_by_one = ctx.hll_new(p, seed=seed)                                # and rising one call at a time
    for j in range(q + 1):
        _add_words(ctx, one_by_one, keys[j:j + 1])
    assert _regs(one_by_one)[3] == 65 - p and np.count_nonzero(_regs(one_by_one)) == 1
    assert int(u64(fresh.histogram())[65 - p]) == int((exp == 65 - p).sum()) >= 1


# ---------------------------------------------------------------- hll_add == add_words over the windows call
@pytest.mark.parametrize("k", (21, 31, 33, 63))
def test_hll_add_equals_add_words_over_the_windows(ctx, k):
    rng = np.random.default_rng(500 + k)
    add = ctx.hll_add if k <= 31 else ctx.hll_add2
    for p in (9, 15):                                                     # a block-private and a global array
        for name, host, n, L, offsets, shift in _read_cases(np.random.default_rng(500 + k), k):
            buf = _dev(ctx, np.concatenate([np.zeros(shift, np.uint8), host, np.zeros(16, np.uint8)]))
            bases = buf[shift:shift + len(host)]
            d_off = None if offsets is None else _dev(ctx, offsets)
            canon, flags = _windows(ctx, bases, n, L, k, offsets=d_off, host_offsets=offsets)
            assert (flags & 1).any(), name
            exp = hl.registers(canon, p, seed=k, flags=flags)
            h = add(ctx.hll_new(p, seed=k), bases, n, L, k, offsets=d_off)
            assert (_regs(h) == exp).all(), (name, k, p)
            via_words = _add_words(ctx, ctx.hll_new(p, seed=k), canon[(flags & 1) != 0])
            assert (_regs(via_words) == exp).all(), (name, k, p)
            if name == "dirty":
                assert ((flags & 1) == 0).any()
    h = ctx.hll_new(9)
    add(h, None, 0, 150, k)                                               # n_reads = 0 leaves the registers untouched
    add(h, _dev(ctx, random_reads(rng, 40 * (k - 1))), 40, k - 1, k)      # so do reads without a window
    assert not _regs(h).any()


# ---------------------------------------------------------------- more keys than one grid sweep; streams; repeats
@pytest.mark.parametrize("p", (9, 14))
def test_past_one_sweep_repeats_and_other_stream(ctx, p):
    import torch

    from kmers_amd.api import Context

    n_cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    sweep = n_cu * _lib.SKETCH_SWEEP_LANES_PER_CU
    n = sweep + sweep // 8 + 77                               # about 3e5 on 256 compute units
    assert _block_private(ctx, n, p) == (p == 9)
    rng = np.random.default_rng(9 + p)
    keys = _keys(rng, n, 1)
    keys2 = np.stack([keys, keys[::-1]], axis=1)
    exp, exp2 = hl.registers(keys, p, seed=1), hl.registers(keys2, p, seed=1)
    a = _add_words(ctx, ctx.hll_new(p, seed=1), keys)
    assert (_regs(a) == exp).all()
    assert (_regs(_add_words(ctx, ctx.hll_new(p, seed=1), keys2)) == exp2).all()
    _add_words(ctx, a, keys)                                  # the same keys again change nothing
    assert (_regs(a) == exp).all()
    other = Context(stream=torch.cuda.Stream())
    try:
        c = _add_words(other, other.hll_new(p, seed=1), keys)
        other.synchronize()
        assert (_regs(c) == exp).all()
    finally:
        other.close()


# ---------------------------------------------------------------- merge and stats
def test_merge_law_and_aliasing(ctx):
    rng = np.random.default_rng(21)
    for p in (4, 12):
        ka, kb = _keys(rng, 20_000, 1), _keys(rng, 31_000, 1)                 # disjoint (random 64-bit keys)
        a, b = _add_words(ctx, ctx.hll_new(p, seed=2), ka), _add_words(ctx, ctx.hll_new(p, seed=2), kb)
        whole = _regs(_add_words(ctx, ctx.hll_new(p, seed=2), np.concatenate([ka, kb])))
        ea, eb = _regs(a), _regs(b)
        assert (hl.merge(ea, eb) == whole).all() and (ea != eb).any()
        assert (_regs(ctx.hll_merge(a, b)) == whole).all()
        assert (_regs(a) == ea).all() and (_regs(b) == eb).all()
        assert ctx.hll_merge(a, b, out=a) is a and (_regs(a) == whole).all()  # d_out aliasing d_a
        a2 = _add_words(ctx, ctx.hll_new(p, seed=2), ka)
        ctx.hll_merge(a2, b, out=b)                                           # d_out aliasing d_b
        assert (_regs(b) == whole).all()
    # any bytes are merged bytewise, not only ranks
    x, y = rng.integers(0, 256, 1 << 10, dtype=np.uint8), rng.integers(0, 256, 1 << 10, dtype=np.uint8)
    hx, hy = ctx.hll_new(10), ctx.hll_new(10)
    hx.regs.copy_(_dev(ctx, x))
    hy.regs.copy_(_dev(ctx, y))
    assert (_regs(ctx.hll_merge(hx, hy)) == np.maximum(x, y)).all()
    with pytest.raises(ValueError):
        ctx.hll_merge(a, ctx.hll_new(12, seed=3))
    with pytest.raises(ValueError):
        ctx.hll_merge(a, ctx.hll_new(11, seed=2))


@pytest.mark.parametrize("p", (4, 9, 16, 21))
def test_stats_one_array_and_two_accumulate(ctx, p):
    rng = np.random.default_rng(31 + p)
    a = _add_words(ctx, ctx.hll_new(p), _keys(rng, 40_000, 1))
    b = _add_words(ctx, ctx.hll_new(p), _keys(rng, 9_000, 1))
    ea, eb = _regs(a), _regs(b)
    one = ctx.hll_stats(a)
    assert one.numel() == 64 and (u64(one) == hl.bins(ea)).all() and int(u64(one).sum()) == 1 << p
    assert (u64(ctx.hll_stats(a, out=one)) == 2 * hl.bins(ea)).all()
    exp3 = np.concatenate([hl.bins(ea), hl.bins(eb), hl.bins(np.maximum(ea, eb))])
    three = ctx.hll_stats(a, b)
    assert three.numel() == 192 and (u64(three) == exp3).all()
    assert (u64(ctx.hll_stats(a, b, out=three)) == 2 * exp3).all()
    assert (_regs(a) == ea).all() and (_regs(b) == eb).all()


def test_compare_two_key_sets_with_a_known_overlap(ctx):
    p, tol = 14, hl.tolerance(14)
    rng = np.random.default_rng(77)
    pool = np.unique(_keys(rng, 300_100, 1))[:300_000]
    rng.shuffle(pool)
    ka, kb = pool[:200_000], pool[150_000:]                                   # |a| = 2e5, |b| = 1.5e5, overlap 5e4, union 3e5
    exact = {"a": 200_000, "b": 150_000, "union": 300_000, "intersection": 50_000}
    ra, rb = hl.registers(ka, p, seed=4), hl.registers(kb, p, seed=4)
    model = [hl.estimate(hl.bins(r), p) for r in (ra, rb, np.maximum(ra, rb))]
    for got, want in zip(model, (200_000, 150_000, 300_000)):                 # on the model first
        assert abs(got - want) / want <= tol
    a, b = _add_words(ctx, ctx.hll_new(p, seed=4), ka), _add_words(ctx, ctx.hll_new(p, seed=4), kb)
    c = ctx.hll_compare(a, b)
    assert [c.a, c.b, c.union] == model                                       # the same bins, the same doubles
    for name in ("a", "b", "union"):
        assert abs(getattr(c, name) - exact[name]) / exact[name] <= tol, name
    # the intersection carries the three errors it is made of
    assert c.intersection == max(c.a + c.b - c.union, 0.0)
    assert abs(c.intersection - exact["intersection"]) <= tol * (exact["a"] + exact["b"] + exact["union"])
    assert c.jaccard == c.intersection / c.union and c.containment_a == c.intersection / c.a and c.containment_b == c.intersection / c.b
    same = ctx.hll_compare(a, a)
    assert same.jaccard == 1.0 and same.containment_a == 1.0 and same.union == c.a
    empty = ctx.hll_compare(ctx.hll_new(p, seed=4), ctx.hll_new(p, seed=4))
    assert (empty.a, empty.union, empty.intersection, empty.jaccard, empty.containment_b) == (0.0, 0.0, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        ctx.hll_compare(a, ctx.hll_new(p, seed=5))


# ---------------------------------------------------------------- a count table's keys; count_solid sized by the estimate
@pytest.mark.parametrize("k", (31, 47))
def test_count_table_keys_estimate_n_distinct(ctx, k):
    rng = np.random.default_rng(700 + k)
    n, L, p = 2000, 150, 14
    host = random_reads(rng, n * L)
    host.reshape(n, L)[::2] = host.reshape(n, L)[1::2]                        # every read twice: half the windows are new
    bases = _dev(ctx, host)
    full, add_words, add = ((ctx.count_canonical, ctx.hll_add_words, ctx.hll_add) if k <= 31 else
                            (ctx.count_canonical2, ctx.hll_add_words2, ctx.hll_add2))
    kmers, counts = full(bases, n, L, k)
    n_distinct = int(counts.numel())
    assert n_distinct > 100_000
    h = add_words(ctx.hll_new(p, seed=3), kmers)
    assert abs(h.estimate() - n_distinct) / n_distinct <= hl.tolerance(p)
    assert (_regs(add(ctx.hll_new(p, seed=3), bases, n, L, k)) == _regs(h)).all()   # the reads hold those keys and no others


@pytest.fixture(scope="module")
def solid_reads():
    return sk.solid_batches(2024)


@pytest.mark.parametrize("k", (31, 47))
def test_count_solid_sizes_its_sketch(ctx, solid_reads, k):
    solid, add, full = ((ctx.count_solid, ctx.hll_add, ctx.count_canonical) if k <= 31 else
                        (ctx.count_solid2, ctx.hll_add2, ctx.count_canonical2))
    batches = [(_dev(ctx, b), len(o) - 1, 160, _dev(ctx, o)) for b, o in solid_reads]
    ek, ec, es = solid(batches, k, 2, log2_blocks=18)
    gk, gc, s = solid(batches, k, 2, log2_blocks=None)
    assert gk.shape == ek.shape and (u64(gk) == u64(ek)).all() and (u64(gc) == u64(ec)).all() and ec.numel() > 10000
    gk, gc, s2 = solid(batches, k, 2)                                         # None is the default
    assert s2.log2_blocks == s.log2_blocks and (u64(gc) == u64(ec)).all()
    h = ctx.hll_new()
    for b in batches:
        add(h, *b[:3], k, offsets=b[3])
    assert s.log2_blocks == h.sketch_log2_blocks() == hl.sketch_log2_blocks(h.estimate())
    fill = s.fill()
    print(f"k={k} estimate={h.estimate():.0f} log2_blocks={s.log2_blocks} fill={fill:.4f}")
    assert fill <= 0.25 + hl.tolerance(14)
    assert s.log2_blocks == 0 or fill > 0.25 / 2 - hl.tolerance(14)           # and no larger than it has to be
    # the estimate is of the distinct k-mers of all batches together
    all_bases = np.concatenate([b for b, _ in solid_reads])
    all_offsets = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(o.astype(np.int64)) for _, o in solid_reads]))]).astype(np.uint64)
    nd = int(full(_dev(ctx, all_bases), len(all_offsets) - 1, 160, k, offsets=_dev(ctx, all_offsets))[1].numel())
    assert abs(h.estimate() - nd) / nd <= hl.tolerance(14)


# ---------------------------------------------------------------- the C++ host layer
def test_cpp_hll_class_against_the_model(tmp_path):
    """kmx::Hll of include/kmx.hpp (tests/cpp/test_hll_hpp.cpp), compiled here and run as a child process: its bins are the model's."""
    import os
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_hll_hpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "test_hll_hpp.cpp"),
                           "-L", os.path.join(root, "kmers_amd"), "-lkmx", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(root, "kmers_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    n, p, seed = 100_000, 12, 9
    r = subprocess.run([exe, str(n), str(p), str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all C++ hll checks passed" in r.stdout, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    with np.errstate(over="ignore"):
        keys = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    whole, half = hl.registers(keys, p, seed=seed), hl.registers(keys[:n // 2], p, seed=seed)
    for line, exp in zip(lines[:3], (whole, half, whole)):
        assert [int(v) for v in line.split()] == [int(v) for v in hl.bins(exp)]
    est, lb, ca, cb, cu = lines[3].split()
    want = hl.estimate(hl.bins(whole), p)
    assert float(est) == float(ca) == float(cb) == float(cu) and abs(float(est) - want) <= 1e-12 * want   # (after the merge both are `all`)
    assert int(lb) == hl.sketch_log2_blocks(want) and abs(want - n) / n <= hl.tolerance(p)


# ---------------------------------------------------------------- argument errors
def test_argument_errors(ctx):
    rng = np.random.default_rng(1)
    lib, hd = ctx.lib, ctx._h
    h = ctx.hll_new(6)
    keys = _dev(ctx, _keys(rng, 64, 1))
    hist = ctx.hll_stats(h)
    bases = _dev(ctx, random_reads(rng, 10 * 150))
    r = ctx._reads(bases, 10, 150, None)
    p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)   # noqa: E731
    before, hist_before = _regs(h).copy(), u64(hist).copy()
    for bad in (3, 25, 0, 64):                        # log2_regs outside 4..24
        assert lib.kmx_hll_add_words(hd, p(keys), 64, p(h.regs), bad, 0) == _lib.E_ARG
        assert lib.kmx_hll_add_words2(hd, p(keys), 32, p(h.regs), bad, 0) == _lib.E_ARG
        assert lib.kmx_hll_add(hd, C.byref(r), 31, p(h.regs), bad, 0) == _lib.E_ARG
        assert lib.kmx_hll_add2(hd, C.byref(r), 47, p(h.regs), bad, 0) == _lib.E_ARG
        assert lib.kmx_hll_merge(hd, p(h.regs), p(h.regs), bad, p(h.regs)) == _lib.E_ARG
        assert lib.kmx_hll_stats(hd, p(h.regs), None, bad, p(hist)) == _lib.E_ARG
        assert lib.kmx_hll_add_words(hd, None, 0, None, bad, 0) == _lib.E_ARG
    # a misaligned array
    assert lib.kmx_hll_add_words(hd, p(keys), 64, p(h.regs, 8), 5, 0) == _lib.E_ARG
    assert lib.kmx_hll_add(hd, C.byref(r), 31, p(h.regs, 1), 5, 0) == _lib.E_ARG
    assert lib.kmx_hll_merge(hd, p(h.regs), p(h.regs, 4), 5, p(h.regs)) == _lib.E_ARG
    assert lib.kmx_hll_merge(hd, p(h.regs), p(h.regs), 5, p(h.regs, 2)) == _lib.E_ARG
    assert lib.kmx_hll_stats(hd, p(h.regs, 8), None, 5, p(hist)) == _lib.E_ARG
    assert lib.kmx_hll_stats(hd, p(h.regs), p(h.regs, 8), 5, p(hist)) == _lib.E_ARG
    # a NULL array with work to do; without work it is a no-op
    assert lib.kmx_hll_add_words(hd, p(keys), 64, None, 6, 0) == _lib.E_ARG
    assert lib.kmx_hll_add2(hd, C.byref(r), 47, None, 6, 0) == _lib.E_ARG
    assert lib.kmx_hll_merge(hd, p(h.regs), None, 6, p(h.regs)) == _lib.E_ARG
    assert lib.kmx_hll_stats(hd, None, None, 6, p(hist)) == _lib.E_ARG
    assert lib.kmx_hll_stats(hd, p(h.regs), None, 6, None) == _lib.E_ARG
    assert lib.kmx_hll_add_words(hd, None, 0, None, 6, 0) == _lib.OK
    assert lib.kmx_hll_add_words(hd, None, 64, p(h.regs), 6, 0) == _lib.E_ARG
    empty = ctx._reads(None, 0, 150, None)
    assert lib.kmx_hll_add(hd, C.byref(empty), 31, None, 6, 0) == _lib.OK
    # k out of range for each width
    for fn in (lib.kmx_hll_add, lib.kmx_hll_add2):
        assert fn(hd, C.byref(r), 32, p(h.regs), 6, 0) == _lib.E_K_RANGE
        assert fn(hd, C.byref(r), 0, p(h.regs), 6, 0) == _lib.E_K_RANGE
        assert fn(hd, C.byref(r), 65, p(h.regs), 6, 0) == _lib.E_K_RANGE
    assert lib.kmx_hll_add(hd, C.byref(r), 33, p(h.regs), 6, 0) == _lib.E_K_RANGE
    assert lib.kmx_hll_add2(hd, C.byref(r), 31, p(h.regs), 6, 0) == _lib.E_K_RANGE
    # a misaligned two-word key array
    assert lib.kmx_hll_add_words2(hd, p(keys, 8), 8, p(h.regs), 6, 0) == _lib.E_ARG
    with pytest.raises(ValueError):
        ctx.hll_new(3)
    with pytest.raises(ValueError):
        ctx.hll_new(25)
    ctx.synchronize()
    assert (_regs(h) == before).all() and (u64(hist) == hist_before).all()
