"""Set algebra and comparison of two count tables on the GPU: kmx_count_setop(2), kmx_count_compare(2) (kmx_count_setop.hip).

Everything is exact (u64 equality, no tolerance).  Pinned to the oracle: two read batches, tables built on the host from the
oracle's canonical words and flags (batches and table_of from tests/count_np.py), thinned independently, one table's counts
multiplied by 1..3; the expected tables are numpy written here (keys of both tables ranked in their union -- two-word keys by
np.unique over (high, low) columns -- and the five operations stated on boolean masks over that union).  Every such test asserts
of its own inputs that a tenth of the union lies in both tables, a tenth only in a, a tenth only in b, and that shared keys fall on
both sides of count_a <= count_b.  Then hand-built tables around the tile boundaries (the tile is _lib.SETOP_TILE merged entries),
the edges of the ABI, and identities between device calls at a size the oracle cannot reach."""
import ctypes as C

import numpy as np
import pytest

from kmers_amd import _lib
from kmers_amd._lib import (RULE_LEFT, RULE_MAX, RULE_MIN, RULE_RIGHT, RULE_SUM, SETOP_COUNTER_SUBTRACT, SETOP_INTERSECT, SETOP_SUBTRACT,
                            SETOP_SYMDIFF, SETOP_TILE, SETOP_UNION)
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import dirty, table_of, two_batches, u64

pytestmark = pytest.mark.gpu

KS1 = (1, 2, 5, 9, 13, 21, 31)
KS2 = (33, 34, 35, 47, 63, 64)
DIRTY_KS = (9, 21, 34, 63)   # batches with 2 % dirty reads; the others are clean
RULES = (RULE_SUM, RULE_MIN, RULE_MAX, RULE_LEFT, RULE_RIGHT)
# every (op, rule) the ABI serves
COMBOS = [(SETOP_INTERSECT, r) for r in RULES] + [(SETOP_UNION, r) for r in RULES] + [(SETOP_SUBTRACT, 0), (SETOP_SYMDIFF, 0),
                                                                                       (SETOP_COUNTER_SUBTRACT, 0)]
T = SETOP_TILE


# ---------------------------------------------------------------- the expected results, on the host
def _rank(ka, kb):
    """(the union's keys ascending, rank of every key of a in it, rank of every key of b)"""
    allk = np.concatenate([ka, kb])
    if allk.ndim == 1:
        u, inv = np.unique(allk, return_inverse=True)
    else:
        u, inv = np.unique(allk[:, ::-1], axis=0, return_inverse=True)   # rows (high, low): the order of a 2k-bit integer
        u = u[:, ::-1]
    inv = np.asarray(inv).reshape(-1)
    return np.ascontiguousarray(u), inv[:len(ka)], inv[len(ka):]


def _spread(ka, ca, kb, cb):
    u, ia, ib = _rank(ka, kb)
    in_a, in_b = np.zeros(len(u), bool), np.zeros(len(u), bool)
    fa, fb = np.zeros(len(u), np.uint64), np.zeros(len(u), np.uint64)
    in_a[ia], in_b[ib] = True, True
    fa[ia], fb[ib] = ca, cb
    return u, in_a, in_b, fa, fb


def _host_setop(op, rule, ka, ca, kb, cb):
    u, in_a, in_b, fa, fb = _spread(ka, ca, kb, cb)
    both = in_a & in_b
    ruled = {RULE_SUM: fa + fb, RULE_MIN: np.minimum(fa, fb), RULE_MAX: np.maximum(fa, fb), RULE_LEFT: fa, RULE_RIGHT: fb}[rule]
    if op == SETOP_INTERSECT:
        m, c = both, ruled
    elif op == SETOP_UNION:
        m, c = in_a | in_b, np.where(both, ruled, fa + fb)   # (a key of one table: the other side is 0)
    elif op == SETOP_SUBTRACT:
        m, c = in_a & ~in_b, fa
    elif op == SETOP_SYMDIFF:
        m, c = in_a ^ in_b, fa + fb
    else:
        m, c = in_a & (~in_b | (fa > fb)), fa - fb
    return u[m], c[m]


def _host_compare(ka, ca, kb, cb):
    u, in_a, in_b, fa, fb = _spread(ka, ca, kb, cb)
    both = in_a & in_b
    s = lambda x: int(np.sum(x, dtype=np.uint64))   # (wraps mod 2^64 as the device adds)
    return dict(n_both=int(both.sum()), n_only_a=int((in_a & ~in_b).sum()), n_only_b=int((in_b & ~in_a).sum()), sum_a=s(fa), sum_b=s(fb),
                sum_a_both=s(fa[both]), sum_b_both=s(fb[both]), sum_min=s(np.minimum(fa, fb)), sum_max=s(np.maximum(fa, fb)))


# ---------------------------------------------------------------- the device calls
def _words(k):
    return k.shape[1] if k.ndim == 2 else 1


def _dev(ctx, x):
    return None if x is None else ctx.to_device(np.ascontiguousarray(x))


def _dev_setop(ctx, op, rule, ka, ca, kb, cb, max_out=None):
    f = ctx.count_setop if _words(ka) == 1 else ctx.count_setop2
    ok, oc = f(op, _dev(ctx, ka), _dev(ctx, ca), _dev(ctx, kb), _dev(ctx, cb), rule, max_out)
    return u64(ok), u64(oc)


def _raw(ctx, op, rule, da, dca, na, db, dcb, nb, ok, oc, max_out, words=1):
    """the C call itself: (status, *h_n_out)"""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    n = C.c_uint64(0xDEAD)
    f = ctx.lib.kmx_count_setop if words == 1 else ctx.lib.kmx_count_setop2
    st = f(ctx._h, op, rule, p(da), p(dca), na, p(db), p(dcb), nb, p(ok), p(oc), max_out, C.byref(n))
    return st, n.value


def _dev_compare(ctx, ka, ca, kb, cb):
    f = ctx.count_compare if _words(ka) == 1 else ctx.count_compare2
    return f(_dev(ctx, ka), _dev(ctx, ca), _dev(ctx, kb), _dev(ctx, cb))


def _same(got, want):
    gk, gc = got
    wk, wc = want
    return gk.shape == wk.shape and gc.shape == wc.shape and (gk == wk).all() and (gc == wc).all()


def _check_all(ctx, ka, ca, kb, cb, tag):
    """every operation, every rule, the forms without counts, the count-only call and the comparison against the host"""
    w = _words(ka)
    da, dca, db, dcb = _dev(ctx, ka), _dev(ctx, ca), _dev(ctx, kb), _dev(ctx, cb)
    f = ctx.count_setop if w == 1 else ctx.count_setop2
    for op, rule in COMBOS:
        wk, wc = _host_setop(op, rule, ka, ca, kb, cb)
        ok, oc = f(op, da, dca, db, dcb, rule)
        assert _same((u64(ok), u64(oc)), (wk, wc)), (tag, op, rule, len(wk), int(oc.numel()))
        st, n = _raw(ctx, op, rule, da if len(ka) else None, dca if len(ka) else None, len(ka), db if len(kb) else None,
                     dcb if len(kb) else None, len(kb), None, None, 0, w)
        assert (st, n) == (_lib.OK, len(wk)), (tag, op, rule, "count only")
    # a count array the operation never reads may be missing
    for op, rule, xa, xb in ((SETOP_SUBTRACT, 0, dca, None), (SETOP_INTERSECT, RULE_LEFT, dca, None), (SETOP_INTERSECT, RULE_RIGHT, None, dcb)):
        ok, oc = f(op, da, xa, db, xb, rule)
        assert _same((u64(ok), u64(oc)), _host_setop(op, rule, ka, ca, kb, cb)), (tag, op, rule, "without counts")
    fc = ctx.count_compare if w == 1 else ctx.count_compare2
    want = _host_compare(ka, ca, kb, cb)
    got = fc(da, dca, db, dcb)
    assert {k: getattr(got, k) for k in want} == want, (tag, "compare")
    got = fc(da, None, db, None)
    want0 = {k: (v if k.startswith("n_") else 0) for k, v in want.items()}
    assert {k: getattr(got, k) for k in want0} == want0, (tag, "compare without counts")


# ---------------------------------------------------------------- 1. pinned to the oracle
def oracle_tables(orc, k, n=3000, L=150):
    """the two tables of the oracle tests at this k: ((keys_a, counts_a), (keys_b, counts_b))"""
    rng = np.random.default_rng(2100 + k)
    a, b = two_batches(rng, n, L)
    rng2 = np.random.default_rng(4200 + k)   # (thinning, dirt and factors from a stream of their own: the batches are those of the seed)
    if k in DIRTY_KS:
        a, b = dirty(a, rng2, 0.02, n, L), dirty(b, rng2, 0.02, n, L)
    f = orc.canonical_windows if k <= 31 else orc.canonical_windows2
    out = []
    for host in (a, b):
        _, _, canon, flags = f(host, n, L, k, offsets=None)
        tk, tc = table_of(np.asarray(canon, np.uint64), np.asarray(flags, np.uint8))
        keep = rng2.random(len(tk)) < 2.0 / 3.0
        out.append((np.ascontiguousarray(tk[keep]), tc[keep]))
    (ka, ca), (kb, cb) = out
    ca = ca * rng2.integers(1, 4, len(ca)).astype(np.uint64)   # counts made unequal: MIN / MAX / LEFT / RIGHT differ
    return (ka, ca), (kb, cb)


def assert_inputs_exercise_every_branch(ka, ca, kb, cb):
    """of the INPUTS: a tenth of the union in both, a tenth only in a, a tenth only in b; shared keys on both sides of count_a <= count_b"""
    if len(ka) < 64 or len(kb) < 64:
        return
    u, in_a, in_b, fa, fb = _spread(ka, ca, kb, cb)
    both = in_a & in_b
    nu, nb_, na_, nb2 = len(u), int(both.sum()), int((in_a & ~in_b).sum()), int((in_b & ~in_a).sum())
    assert 10 * nb_ >= nu and 10 * na_ >= nu and 10 * nb2 >= nu, (nu, nb_, na_, nb2)
    assert int((fa[both] <= fb[both]).sum()) >= 1 and int((fa[both] > fb[both]).sum()) >= 1


@pytest.mark.parametrize("k", KS1 + KS2)
def test_setops_and_compare_against_the_oracle(ctx, orc, k):
    (ka, ca), (kb, cb) = oracle_tables(orc, k)
    assert_inputs_exercise_every_branch(ka, ca, kb, cb)
    _check_all(ctx, ka, ca, kb, cb, k)
    _check_all(ctx, kb, cb, ka, ca, (k, "swapped"))


# ---------------------------------------------------------------- 2. tile boundaries
def _keys_w1(v):
    return v.astype(np.uint64) * np.uint64(3) + np.uint64(1)


def _keys_hi(v):   # two-word keys that differ only in the high word
    v = v.astype(np.uint64)
    return np.stack([np.full(len(v), 0x8000000000000005, np.uint64), v], axis=1)


def _keys_lo(v):   # ... only in the low word, which crosses bit 63 inside the table (unsigned order)
    v = v.astype(np.uint64)
    return np.stack([v + np.uint64(2**63 - 3000), np.full(len(v), 7, np.uint64)], axis=1)


def _keys_mixed(v):   # three low words per high word: 1, 2^63, 2^64 - 1
    v = v.astype(np.uint64)
    lo = np.array([1, 2**63, 2**64 - 1], np.uint64)[(v % np.uint64(3)).astype(np.int64)]
    return np.stack([lo, v // np.uint64(3)], axis=1)


SHAPES = (_keys_w1, _keys_hi, _keys_lo, _keys_mixed)
SIZES = (T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 7)


def _counts(rng, n):
    return rng.integers(1, 1000, n).astype(np.uint64)


def _run_values(ctx, shape, va, vb, rng, tag):
    va, vb = np.asarray(va, np.int64), np.asarray(vb, np.int64)
    _check_all(ctx, shape(va), _counts(rng, len(va)), shape(vb), _counts(rng, len(vb)), (shape.__name__,) + tuple(tag))


@pytest.mark.parametrize("shape", SHAPES)
def test_tile_boundaries_hand_built_tables(ctx, shape):
    rng = np.random.default_rng(77)
    for n in SIZES:
        v = np.arange(n)
        _run_values(ctx, shape, v, v, rng, ("a == b", n))
        _run_values(ctx, shape, 2 * v, 2 * v + 1, rng, ("interleaved", n))
        _run_values(ctx, shape, v, v + n, rng, ("a below b", n))
        _run_values(ctx, shape, v + n, v, rng, ("b below a", n))
        for one in (0, n // 2, n - 1):               # a single key inside the other table: first, middle, last
            _run_values(ctx, shape, [one], v, rng, ("one key of a, shared", n, one))
            _run_values(ctx, shape, v, [one], rng, ("one key of b, shared", n, one))
        for one in (0, n, 2 * n):                    # ... and between its keys: before, middle, behind
            _run_values(ctx, shape, [one], 2 * v + 1, rng, ("one key of a, absent", n, one))
            _run_values(ctx, shape, 2 * v + 1, [one], rng, ("one key of b, absent", n, one))


def _tables_with_pairs_at(pair_starts, n_merged, rng):
    """values of a and of b whose merged sequence (ties: a first) holds a shared pair at positions p, p + 1 for every p given; the
    other positions hold keys of one table only"""
    va, vb, pos, v = [], [], 0, 0
    while pos < n_merged:
        if pos in pair_starts:
            va.append(v)
            vb.append(v)
            pos += 2
        else:
            (va if rng.random() < 0.5 else vb).append(v)
            pos += 1
        v += 1
    return va, vb


@pytest.mark.parametrize("shape", SHAPES)
def test_shared_pairs_on_the_tile_boundaries(ctx, shape):
    """a shared pair at the merged positions m T - 1, m T (a's entry the last of one tile, b's the first of the next) for the first
    three boundaries -- together and one boundary at a time --, and one position to either side"""
    rng = np.random.default_rng(78)
    for shift in (-1, 0, -2):
        starts = [m * T + shift for m in (1, 2, 3)]
        for chosen in ([starts[0]], [starts[1]], [starts[2]], starts):
            va, vb = _tables_with_pairs_at(set(chosen), 3 * T + 50, rng)
            # the construction puts the pairs where it says: merged with a first, positions p and p + 1 hold one value
            merged = np.sort(np.concatenate([2 * np.asarray(va), 2 * np.asarray(vb) + 1]))
            for p in chosen:
                assert merged[p] // 2 == merged[p + 1] // 2 and merged[p] % 2 == 0
            _run_values(ctx, shape, va, vb, rng, ("pairs at", tuple(chosen)))
    # runs of shared keys across each boundary: every second merged position around m T starts a pair, in both phases
    for phase in (0, 1):
        starts = {m * T - 8 + phase + 2 * i for m in (1, 2, 3) for i in range(8)}
        va, vb = _tables_with_pairs_at(starts, 3 * T + 50, rng)
        _run_values(ctx, shape, va, vb, rng, ("runs of pairs", phase))


# ---------------------------------------------------------------- 3. edges
@pytest.mark.parametrize("shape", (_keys_w1, _keys_mixed))
def test_empty_tables(ctx, shape):
    rng = np.random.default_rng(79)
    v, none = np.arange(T + 5), np.arange(0)
    _run_values(ctx, shape, none, v, rng, ("a empty",))
    _run_values(ctx, shape, v, none, rng, ("b empty",))
    _run_values(ctx, shape, none, none, rng, ("both empty",))
    # ... given as NULL pointers
    w = 1 if shape is _keys_w1 else 2
    for op, rule in COMBOS:
        assert _raw(ctx, op, rule, None, None, 0, None, None, 0, None, None, 0, w) == (_lib.OK, 0)
    rec = _lib.TableCompare(*([9] * 9))
    f = ctx.lib.kmx_count_compare if w == 1 else ctx.lib.kmx_count_compare2
    assert f(ctx._h, None, None, 0, None, None, 0, C.byref(rec)) == _lib.OK
    assert [getattr(rec, n) for n, _ in rec._fields_] == [0] * 9


@pytest.mark.parametrize("shape", (_keys_w1, _keys_mixed))
def test_max_out_and_sentinels(ctx, shape):
    import torch

    rng = np.random.default_rng(80)
    va, vb = _tables_with_pairs_at({5, 100, T - 1, 2 * T}, 2 * T + 300, rng)
    ka, kb = shape(np.asarray(va)), shape(np.asarray(vb))
    ca, cb = _counts(rng, len(ka)), _counts(rng, len(kb))
    w = _words(ka)
    da, dca, db, dcb = _dev(ctx, ka), _dev(ctx, ca), _dev(ctx, kb), _dev(ctx, cb)
    for op, rule in COMBOS:
        wk, wc = _host_setop(op, rule, ka, ca, kb, cb)
        n_out = len(wk)
        assert n_out >= 2
        ok = torch.full((w * (n_out + 8),), -1, dtype=torch.int64, device=ctx.device)
        oc = torch.full((n_out + 8,), -1, dtype=torch.int64, device=ctx.device)
        # one entry short: KMX_E_NOMEM, the size reported, nothing written
        assert _raw(ctx, op, rule, da, dca, len(ka), db, dcb, len(kb), ok, oc, n_out - 1, w) == (_lib.E_NOMEM, n_out)
        assert (ok == -1).all() and (oc == -1).all()
        # exactly enough: served, and nothing behind the result is touched
        assert _raw(ctx, op, rule, da, dca, len(ka), db, dcb, len(kb), ok, oc, n_out, w) == (_lib.OK, n_out)
        assert (u64(ok[:w * n_out]).reshape(wk.shape) == wk).all() and (u64(oc[:n_out]) == wc).all()
        assert (ok[w * n_out:] == -1).all() and (oc[n_out:] == -1).all()
        # one output without the other; a count array the operation reads missing
        assert _raw(ctx, op, rule, da, dca, len(ka), db, dcb, len(kb), ok, None, n_out, w)[0] == _lib.E_ARG
        assert _raw(ctx, op, rule, da, dca, len(ka), db, dcb, len(kb), None, oc, n_out, w)[0] == _lib.E_ARG
        reads_a = not (op == SETOP_INTERSECT and rule == RULE_RIGHT)
        reads_b = not (op == SETOP_SUBTRACT or (op == SETOP_INTERSECT and rule == RULE_LEFT))
        assert (_raw(ctx, op, rule, da, None, len(ka), db, dcb, len(kb), ok, oc, n_out, w)[0] == _lib.E_ARG) == reads_a
        assert (_raw(ctx, op, rule, da, dca, len(ka), db, None, len(kb), ok, oc, n_out, w)[0] == _lib.E_ARG) == reads_b
    # the comparison takes the counts of both tables or of neither
    rec = _lib.TableCompare()
    f = ctx.lib.kmx_count_compare if w == 1 else ctx.lib.kmx_count_compare2
    p = lambda t: C.c_void_p(t.data_ptr())
    assert f(ctx._h, p(da), p(dca), len(ka), p(db), None, len(kb), C.byref(rec)) == _lib.E_ARG
    assert f(ctx._h, p(da), None, len(ka), p(db), p(dcb), len(kb), C.byref(rec)) == _lib.E_ARG
    assert f(ctx._h, p(da), p(dca), 2**40 + 1, p(db), p(dcb), len(kb), C.byref(rec)) == _lib.E_ARG


def test_misaligned_two_word_keys(ctx):
    import torch

    rng = np.random.default_rng(81)
    v = np.arange(300)
    ka, kb = _keys_mixed(2 * v), _keys_mixed(3 * v)
    ca, cb = _counts(rng, 300), _counts(rng, 300)
    pad = lambda k: ctx.to_device(np.concatenate([np.zeros(1, np.uint64), k.reshape(-1)]))[1:]   # 8 bytes off a 16-byte boundary
    da, db, dca, dcb = ctx.to_device(ka), ctx.to_device(kb), ctx.to_device(ca), ctx.to_device(cb)
    ok = torch.full((2 * 600 + 1,), -1, dtype=torch.int64, device=ctx.device)
    oc = torch.full((600,), -1, dtype=torch.int64, device=ctx.device)
    assert pad(ka).data_ptr() % 16 == 8 and ok[1:].data_ptr() % 16 == 8
    assert _raw(ctx, SETOP_UNION, 0, pad(ka), dca, 300, db, dcb, 300, ok, oc, 600, 2)[0] == _lib.E_ARG
    assert _raw(ctx, SETOP_UNION, 0, da, dca, 300, pad(kb), dcb, 300, ok, oc, 600, 2)[0] == _lib.E_ARG
    assert _raw(ctx, SETOP_UNION, 0, da, dca, 300, db, dcb, 300, ok[1:], oc, 600, 2)[0] == _lib.E_ARG
    assert (ok == -1).all() and (oc == -1).all()
    rec = _lib.TableCompare()
    p = lambda t: C.c_void_p(t.data_ptr())
    assert ctx.lib.kmx_count_compare2(ctx._h, p(pad(ka)), p(dca), 300, p(db), p(dcb), 300, C.byref(rec)) == _lib.E_ARG
    assert ctx.lib.kmx_count_compare2(ctx._h, p(da), p(dca), 300, p(pad(kb)), p(dcb), 300, C.byref(rec)) == _lib.E_ARG
    assert _raw(ctx, SETOP_UNION, 0, da, dca, 300, db, dcb, 300, ok[:1200], oc, 600, 2)[0] == _lib.OK


@pytest.mark.parametrize("shape", (_keys_w1, _keys_mixed))
def test_sum_wraps_exactly_as_count_merge(ctx, shape):
    rng = np.random.default_rng(82)
    v = np.arange(T + 40)
    ka, kb = shape(v), shape(v[::2])
    ca = rng.integers(2**64 - 50, 2**64, len(ka), dtype=np.uint64)
    cb = rng.integers(1, 100, len(kb), dtype=np.uint64)
    want = _host_setop(SETOP_UNION, RULE_SUM, ka, ca, kb, cb)
    assert (want[1] < 100).any() and (want[1] > 2**63).any()   # some sums wrapped, some did not
    assert _same(_dev_setop(ctx, SETOP_UNION, RULE_SUM, ka, ca, kb, cb), want)
    merge = ctx.count_merge if _words(ka) == 1 else ctx.count_merge2
    mk, mc = merge(_dev(ctx, ka), _dev(ctx, ca), _dev(ctx, kb), _dev(ctx, cb))
    assert _same((u64(mk), u64(mc)), want)
    got = _dev_compare(ctx, ka, ca, kb, cb)
    assert {k: getattr(got, k) for k in ("sum_a", "sum_max", "sum_min")} == {k: _host_compare(ka, ca, kb, cb)[k] for k in ("sum_a", "sum_max", "sum_min")}


def _setop_bytes(n):
    """kmx.h: 16 * (tiles + 1) bytes rounded up to 256 plus 8 * (tiles + 2) bytes rounded up to 256, tiles = ceil(n / 2048)"""
    tiles = -(-n // 2048)
    up = lambda b: (b + 255) // 256 * 256
    return up(16 * (tiles + 1)) + up(8 * (tiles + 2))


@pytest.mark.parametrize("shape", (_keys_w1, _keys_mixed))
def test_work_buffer_limit_is_the_documented_formula(ctx, shape):
    import torch

    rng = np.random.default_rng(83)
    va, vb = _tables_with_pairs_at({T - 1, 7 * T}, 40 * T + 11, rng)
    ka, kb = shape(np.asarray(va)), shape(np.asarray(vb))
    ca, cb = _counts(rng, len(ka)), _counts(rng, len(kb))
    w, n = _words(ka), len(ka) + len(kb)
    need = _setop_bytes(n)
    assert need == 256 * 3 + 256 * 2      # 41 tiles: 672 bytes of cuts, 344 bytes of totals
    da, dca, db, dcb = _dev(ctx, ka), _dev(ctx, ca), _dev(ctx, kb), _dev(ctx, cb)
    ok = torch.full((w * n,), -1, dtype=torch.int64, device=ctx.device)
    oc = torch.full((n,), -1, dtype=torch.int64, device=ctx.device)
    rec = _lib.TableCompare(*([9] * 9))
    fc = ctx.lib.kmx_count_compare if w == 1 else ctx.lib.kmx_count_compare2
    p = lambda t: C.c_void_p(t.data_ptr())
    try:
        ctx.set_work_buffer_limit(need - 1)
        allocs0 = ctx.work_buffer_info()[1]
        st, got = _raw(ctx, SETOP_UNION, RULE_SUM, da, dca, len(ka), db, dcb, len(kb), ok, oc, n, w)
        assert st == _lib.E_NOMEM
        assert fc(ctx._h, p(da), p(dca), len(ka), p(db), p(dcb), len(kb), C.byref(rec)) == _lib.E_NOMEM
        assert ctx.work_buffer_info()[1] == allocs0          # refused before the buffer was touched: nothing ran
        assert (ok == -1).all() and (oc == -1).all() and rec.n_both == 9
        ctx.set_work_buffer_limit(need)
        wk, wc = _host_setop(SETOP_UNION, RULE_SUM, ka, ca, kb, cb)
        assert _raw(ctx, SETOP_UNION, RULE_SUM, da, dca, len(ka), db, dcb, len(kb), ok, oc, n, w) == (_lib.OK, len(wk))
        assert (u64(ok[:w * len(wk)]).reshape(wk.shape) == wk).all() and (u64(oc[:len(wk)]) == wc).all()
        assert fc(ctx._h, p(da), p(dca), len(ka), p(db), p(dcb), len(kb), C.byref(rec)) == _lib.OK
        assert rec.n_both == _host_compare(ka, ca, kb, cb)["n_both"]
    finally:
        ctx.set_work_buffer_limit(0)


@pytest.mark.parametrize("k", (31, 47))
def test_repeated_calls_are_bit_identical(ctx, orc, k):
    (ka, ca), (kb, cb) = oracle_tables(orc, k)
    for op, rule in COMBOS:
        first = _dev_setop(ctx, op, rule, ka, ca, kb, cb)
        assert _same(_dev_setop(ctx, op, rule, ka, ca, kb, cb), first), (k, op, rule)
    assert _dev_compare(ctx, ka, ca, kb, cb) == _dev_compare(ctx, ka, ca, kb, cb)


def test_unsorted_tables_stay_inside_the_arrays(ctx):
    """wrong answers are allowed, an access outside the arrays is not.  The cuts of unsorted tables need not ascend, so tiles may
    overlap and the "result" may even be longer than n_a + n_b -- at most 9 entries per thread of every tile (kmx_count_setop.hip:
    a walk is SETOP_IPT + 1 steps).  With room for that: the call succeeds, every key written is a key of an input, and what lies
    behind n_out keeps its sentinel.  With room for n_a + n_b only: the same n_out, and KMX_E_NOMEM with nothing written where it
    does not fit."""
    import torch

    rng = np.random.default_rng(84)
    n = 3 * T + 17
    ka, kb = rng.integers(0, 5000, n).astype(np.uint64), rng.integers(0, 5000, n).astype(np.uint64)   # unsorted, with repeats
    ca, cb = _counts(rng, n), _counts(rng, n)
    da, dca, db, dcb = _dev(ctx, ka), _dev(ctx, ca), _dev(ctx, kb), _dev(ctx, cb)
    tiles = -(-2 * n // T)
    room = tiles * (T // 8) * 9
    for op, rule in COMBOS:
        ok = torch.full((room + 64,), -1, dtype=torch.int64, device=ctx.device)
        oc = torch.full((room + 64,), -1, dtype=torch.int64, device=ctx.device)
        st, n_out = _raw(ctx, op, rule, da, dca, n, db, dcb, n, ok, oc, room, 1)
        assert st == _lib.OK and n_out <= room, (op, rule, st, n_out)
        assert np.isin(u64(ok[:n_out]), np.concatenate([ka, kb])).all()
        assert (ok[n_out:] == -1).all() and (oc[n_out:] == -1).all()
        ok.fill_(-1)
        oc.fill_(-1)
        st2, n_out2 = _raw(ctx, op, rule, da, dca, n, db, dcb, n, ok, oc, 2 * n, 1)
        assert n_out2 == n_out and st2 == (_lib.OK if n_out <= 2 * n else _lib.E_NOMEM), (op, rule, st2, n_out2)
        assert (ok[min(n_out, 2 * n) if st2 == _lib.OK else 0:] == -1).all() and (oc[min(n_out, 2 * n) if st2 == _lib.OK else 0:] == -1).all()
    ctx.count_compare(da, dca, db, dcb)


# ---------------------------------------------------------------- 4. identities at a size the oracle cannot reach
def _device_batches(ctx, n, L, seed):
    import torch

    g = torch.Generator(device=ctx.device)
    g.manual_seed(seed)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=ctx.device)
    a = lut[torch.randint(0, 4, (n, L), generator=g, device=ctx.device)]
    b = lut[torch.randint(0, 4, (n, L), generator=g, device=ctx.device)]
    b[::2] = a[::2]                                  # half of B's reads are reads of A
    return a.reshape(-1).contiguous(), b.reshape(-1).contiguous()


@pytest.mark.parametrize("k,n", ((31, 2_000_000), (47, 1_000_000)))
def test_identities_between_device_calls_at_full_size(ctx, k, n):
    """k = 31: 2.4e8 entries per table (3.9 GB each with its counts), unions of 3.6e8; the peak is the union / merge step -- two
    input tables (7.7 GB as the buffers count_canonical sized), two outputs sized n_a + n_b (15.5 GB) and the merge's work buffer
    (7.7 GB): about 32 GB.  k = 47: 1.04e8 entries per table of 24 bytes, about 21 GB at the same step.  Both fit the automatic
    work-buffer cap of the full-size count tests (count_canonical itself needs 4.8 GB / 3.7 GB of it)."""
    import torch

    L, w = 150, 1 if k <= 31 else 2
    two = "" if w == 1 else "2"
    call = lambda name: getattr(ctx, name + two)
    ba, bb = _device_batches(ctx, n, L, 5000 + k)
    ka, ca = call("count_canonical")(ba, n, L, k)
    kb, cb = call("count_canonical")(bb, n, L, k)
    ka, ca, kb, cb = ka.clone(), ca.clone(), kb.clone(), cb.clone()   # (the tables alone, not the buffers sized to the windows)
    del ba, bb
    torch.cuda.empty_cache()
    na, nb = int(ca.numel()), int(cb.numel())
    setop, merge, lookup, compare = call("count_setop"), call("count_merge"), call("count_lookup"), call("count_compare")
    eq = lambda x, y: x[0].shape == y[0].shape and torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    total = lambda c: int(c.sum().item()) % 2**64

    # UNION / SUM is kmx_count_merge, bit for bit
    un = setop(SETOP_UNION, ka, ca, kb, cb, RULE_SUM)
    mg = merge(ka, ca, kb, cb)
    assert eq(un, mg)
    n_union = int(un[1].numel())
    assert 0 < n_union < na + nb
    # COUNTER_SUBTRACT(merge(a, b), b) == a
    back = setop(SETOP_COUNTER_SUBTRACT, mg[0], mg[1], kb, cb, 0)
    assert eq(back, (ka, ca))
    del un, mg, back
    torch.cuda.empty_cache()

    # INTERSECT / LEFT and SUBTRACT split a; merged, they give it back
    il = setop(SETOP_INTERSECT, ka, ca, kb, None, RULE_LEFT)
    sb = setop(SETOP_SUBTRACT, ka, ca, kb, None, 0)
    n_both = int(il[1].numel())
    assert n_both + int(sb[1].numel()) == na and 10 * n_both >= na and 10 * int(sb[1].numel()) >= na
    assert eq(merge(il[0], il[1], sb[0], sb[1]), (ka, ca))
    # INTERSECT / RIGHT is the entries of b that a holds (lookup membership + boolean indexing)
    ir = setop(SETOP_INTERSECT, ka, None, kb, cb, RULE_RIGHT)
    member = lookup(ka, None, k, kb) != 0
    assert eq(ir, (kb[member], cb[member]))
    del member
    # the comparison's record against the sizes and sums of those tables
    rec = compare(ka, ca, kb, cb)
    assert (rec.n_both, rec.n_only_a, rec.n_only_b) == (n_both, na - n_both, nb - n_both)
    assert n_union == na + nb - n_both
    assert (rec.sum_a, rec.sum_b, rec.sum_a_both, rec.sum_b_both) == (total(ca), total(cb), total(il[1]), total(ir[1]))
    mn = setop(SETOP_INTERSECT, ka, ca, kb, cb, RULE_MIN)
    assert rec.sum_min == total(mn[1])
    del mn, il, ir, sb
    torch.cuda.empty_cache()
    mx = setop(SETOP_UNION, ka, ca, kb, cb, RULE_MAX)
    assert rec.sum_max == total(mx[1]) and int(mx[1].numel()) == n_union
    sets = compare(ka, None, kb, None)
    assert (sets.n_both, sets.n_only_a, sets.n_only_b, sets.sum_a, sets.sum_max) == (n_both, na - n_both, nb - n_both, 0, 0)
