"""Every arm of kmx_canonical_windows and kmx_canonical_windows2 where a wave (a lane) takes several units, every slot checked.

tests/windows_np.py restates the launchers' routing (arm_of), names every arm (ARMS) and builds, for the device's number of compute
units, a batch of U + U // 3 + 6 units and a partial last tile for each case -- U the most units one launch of the arm can hold at
once -- so that at least U // 3 + 6 units are some wave's second or later one: the ring and the lb[] registers of the sinks, the
prefetched rows and their ticket, the STAGE block and the per-lane posF / qF / aF of windows2_tiled_kernel, the grid-stride loops of
the lane-per-read kernels and the mask groups of the ZERO sweep all outlive a unit there.  tests/test_windows_np.py (CPU) shows
that the cases name every arm and that none could pass with a kernel that stops after its first launch's worth, writes a unit with
an earlier unit's words or stores it at an earlier unit's slots.

Every call goes through the C ABI.  The batch repeats a block of P reads, P a prime above the number of tiles; it is laid out on the
device from the block (uniform reads: the buffer ends with the last base, the first base c.lead bytes past a 16-byte boundary).  Every
requested output is the interior of a buffer of 0xA5 bytes with guards on either side; an output that is not requested is NULL.
After the call the status and kmx_ctx_synchronize are KMX_OK, the guards are intact and the interior equals the oracle's arrays for
the block, repeated -- compared on the device, every slot, no tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import elem_np as E
from tests import windows_np as M
from tests.test_gpu_elem_sweep import Env

pytestmark = pytest.mark.gpu

POISON_I64 = E.POISON_U64 - (1 << 64)


@pytest.fixture(scope="module")
def env():
    from kmers_amd.api import Context

    ctx = Context(0)
    yield Env(ctx)
    ctx.close()


def n_cu_of(env) -> int:
    return env.S // (16 * 256)


@functools.lru_cache(maxsize=2)
def _built(case: M.P, n_cu: int, size=None, clean=False) -> M.Built:
    return M.build(case, n_cu, size=size, clean=clean)


def _vp(x):
    return C.c_void_p(x) if x else None


def _repeat_into(dst, blk):
    """dst = the block, over and over"""
    B = len(blk)
    q, rem = divmod(len(dst), B)
    if q:
        dst[: q * B].view(q, B).copy_(blk.unsqueeze(0).expand(q, B))
    if rem:
        dst[q * B:].copy_(blk[:rem])


def _periodic(env, table, n, period):
    """entries 0 .. n of a block table (offsets, first slots) continued with the block's period -> i64 tensor on the device"""
    torch = env.torch
    t = env.ctx.to_device(np.ascontiguousarray(table, np.int64))
    r = torch.arange(n + 1, device=t.device, dtype=torch.int64)
    return (r // period) * int(table[-1]) + t[r % period]


def launch(env, b: M.Built):
    """the batch and the poisoned outputs on the device, the call -> (status, status of kmx_ctx_synchronize, {name: (tensor, lead, elements)})"""
    from kmers_amd import _lib

    torch, c, dev = env.torch, b.case, env.ctx.device
    total = b.total_bytes
    buf = torch.empty(c.lead + (total if total else 16), dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    _repeat_into(buf[c.lead: c.lead + total], env.ctx.to_device(b.bases))
    d_off = d_win = None
    if c.ragged:
        d_off, d_win = _periodic(env, b.off, b.n, b.period), _periodic(env, b.win, b.n, b.period)
    outs, ptr = {}, dict.fromkeys(M.NAMES)
    for nm in c.want:
        if nm == "flags":
            lead, n_el = E.GUARD_BYTES + c.flags_shift, b.total
            t = torch.full((lead + n_el + E.GUARD_BYTES,), E.POISON_U8, dtype=torch.uint8, device=dev)
            ptr[nm] = t.data_ptr() + lead
            assert ptr[nm] % 16 == c.flags_shift
        else:
            lead, n_el = E.GUARD_WORDS + c.words_shift // 8, b.per_slot(nm) * b.total
            t = torch.full((lead + n_el + E.GUARD_WORDS,), POISON_I64, dtype=torch.int64, device=dev)
            ptr[nm] = t.data_ptr() + 8 * lead
            assert ptr[nm] % 16 == c.words_shift
        outs[nm] = (t, lead, n_el)
    r = _lib.Reads(buf.data_ptr() + c.lead, b.n, c.L, d_off.data_ptr() if c.ragged else None)
    fn = env.lib.kmx_canonical_windows2 if b.two else env.lib.kmx_canonical_windows
    st = fn(env.h, C.byref(r), _vp(d_win.data_ptr()) if c.ragged else None, c.k, _vp(ptr["fw"]), _vp(ptr["rc"]), _vp(ptr["canon"]), _vp(ptr["flags"]))
    sync = env.lib.kmx_ctx_synchronize(env.h)
    del buf, d_off, d_win
    return st, sync, outs


def check(env, b: M.Built, outs, what=""):
    """guards intact, every element of every interior as expected -- on the device; a mismatch is read back and reported"""
    torch = env.torch
    for nm, (t, lead, n_el) in outs.items():
        poison = E.POISON_U8 if nm == "flags" else POISON_I64
        assert bool((t[:lead] == poison).all()) and bool((t[lead + n_el:] == poison).all()), (what, b.case.id, f"guards of d_{nm}")
        e = b.exp[nm]
        blk = env.ctx.to_device(e.view(np.int64) if e.dtype == np.uint64 else e)
        inner, Bn = t[lead: lead + n_el], len(e)
        q, rem = divmod(n_el, Bn)
        good = (not q or bool((inner[: q * Bn].view(q, Bn) == blk.unsqueeze(0)).all())) and (not rem or bool((inner[q * Bn:] == blk[:rem]).all()))
        if good:
            continue
        full = torch.empty_like(inner)
        _repeat_into(full, blk)
        wrong = torch.nonzero(inner != full).reshape(-1)
        m = b.per_slot(nm)
        el = int(wrong[0])
        read, unit, late = b.where(el // m)
        unwritten = int((inner == poison).sum())
        pytest.fail(f"{what} {b.case.id}: d_{nm}: {len(wrong)} of {n_el} elements differ ({unwritten} still hold poison); the first is element {el} "
                    f"= slot {el // m} of read {read} (tile {read // 64}), unit {unit} -- {'past' if late else 'within'} U = {b.U} of {b.units} units: "
                    f"{int(inner[el]) & E.M64:#x}, expected {int(full[el]) & E.M64:#x}")


def run(env, b: M.Built, what=""):
    st, sync, outs = launch(env, b)
    assert st == M.OK, (what, b.case.id, b.n, st, env.lib.kmx_last_error(env.h))
    assert sync == M.OK, (what, b.case.id, b.n, sync, env.lib.kmx_last_error(env.h))
    assert set(outs) == set(b.case.want)
    check(env, b, outs, what)
    return outs


# ------------------------------------------------------------------ every arm past what one launch holds, and at the edges

@pytest.mark.parametrize("i", range(len(M.CASES)), ids=[c.id for c in M.CASES])
def test_past_one_sweep(env, i):
    b = _built(M.CASES[i], n_cu_of(env))
    assert b.units >= M.past(b.U) > b.U and set(b.arm.names) <= set(M.ARMS)
    print(f"\n{b.case.id}: {b.n} reads, {-(-b.n // 64)} tiles, {b.units} units (U = {b.U}), block of {b.period} reads, {b.footprint() / 2**20:.0f} MiB")
    run(env, b)


@pytest.mark.parametrize("i", range(len(M.EDGE)), ids=[c.id for c in M.EDGE])
def test_edge_sizes(env, i):
    """1, 63, 64, 65 reads and exactly U units"""
    for size in M.SIZES:
        run(env, M.build(M.EDGE[i], n_cu_of(env), size=size), what=size)


@pytest.mark.parametrize("i", range(len(M.DIRTY_THEN_CLEAN)), ids=[c.id for c in M.DIRTY_THEN_CLEAN])
def test_dirty_then_clean_on_one_context(env, i):
    """a dirty batch past one sweep, then a clean one of the same shape on the SAME context: the masks and the marked count were put back"""
    c = M.DIRTY_THEN_CLEAN[i]
    dirty, clean = _built(c, n_cu_of(env)), M.build(c, n_cu_of(env), clean=True)
    assert dirty.dirty_reads()[dirty.first_read_of_unit(dirty.U):].any() and not clean.dirty.any() and clean.n == dirty.n
    run(env, dirty, "dirty")
    run(env, clean, "clean")
    run(env, dirty, "dirty again")


@pytest.mark.parametrize("i", range(len(M.REPEAT)), ids=[c.id for c in M.REPEAT])
def test_repeat_is_identical(env, i):
    """twice into freshly poisoned buffers: bit-equal"""
    b = _built(M.REPEAT[i], n_cu_of(env))
    first, again = run(env, b, "first"), run(env, b, "again")
    for nm in b.case.want:
        assert first[nm][0].data_ptr() != again[nm][0].data_ptr() and env.torch.equal(first[nm][0], again[nm][0]), nm
