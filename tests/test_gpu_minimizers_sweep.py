"""Every arm of the minimizer calls -- kmx_minimizers, kmx_seqvec_minimizers, kmx_minimizer_words and their _sip13 forms -- past one
grid sweep, exactly.

tests/minimizers_np.py restates the launchers' routing (arm_of), names every arm (ARMS) and builds, for the device's number of
compute units, a batch of U + U // 3 + 1 + 5 units for each case (U = one capped grid of the arm): some blocks take two loop
iterations, some one, the last block is partial.  tests/test_minimizers_np.py (CPU) shows that the cases name every arm and that none
of them could pass with a kernel that stops after one sweep or works on the previous sweep's unit again.

Every call goes through the C ABI.  d_word and d_pos are the interior of poisoned buffers with guards on either side; after the call
the status and *h_first_bad are as expected, the guards are intact and the interior equals the numpy reference -- every slot, no
tolerance: win_offsets is dense, so a slot that keeps its poison is a slot some read owns and nobody wrote.  After
KMX_E_INVALID_BASE the outputs are unspecified (include/kmx.h): the status, *h_first_bad and the guards are checked."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import elem_np as E
from tests import minimizers_np as M
from tests.test_gpu_elem_sweep import Env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from kmers_amd.api import Context

    ctx = Context(0)
    yield Env(ctx)
    ctx.close()


def n_cu_of(env) -> int:
    return env.S // (16 * 256)


@functools.lru_cache(maxsize=2)
def _built(i: int, n_cu: int) -> M.Built:
    return M.build(M.CASES[i], n_cu)


def _vp(x):
    return C.c_void_p(x) if x else None


def call(env, b: M.Built, d: dict):
    """the C ABI call of the batch on the device addresses d -> (status, *h_first_bad or None)"""
    from kmers_amd import _lib

    L, h, c = env.lib, env.h, b.case
    sip = c.hasher == "sip"
    hasher = E.HASH_LEX if c.hasher == "lex" else E.HASH_IDENTITY
    word, pos = _vp(d["word"]), _vp(d["pos"])
    if c.call == "minimizer_words":
        if sip:
            return L.kmx_minimizer_words_sip13(h, _vp(d["words"]), b.n, c.k, c.w, *M.SIP_KEY, word, pos), None
        return L.kmx_minimizer_words(h, _vp(d["words"]), b.n, c.k, c.w, hasher, c.hk, word, pos), None
    if c.call == "seqvec_minimizers":
        if sip:
            return L.kmx_seqvec_minimizers_sip13(h, _vp(d["words"]), b.n, c.L, c.k, c.w, *M.SIP_KEY, word, pos), None
        return L.kmx_seqvec_minimizers(h, _vp(d["words"]), b.n, c.L, c.k, c.w, hasher, c.hk, word, pos), None
    r = _lib.Reads(d["bases"], b.n, c.L, d.get("offsets"))
    fb = C.c_uint64(0x1234)
    if sip:
        return L.kmx_minimizers_sip13(h, C.byref(r), _vp(d.get("win_offsets")), c.k, c.w, *M.SIP_KEY, word, pos, C.byref(fb)), fb.value
    return L.kmx_minimizers(h, C.byref(r), _vp(d.get("win_offsets")), c.k, c.w, hasher, c.hk, word, pos, C.byref(fb)), fb.value


def launch(env, b: M.Built):
    """inputs up (the bases or words c.shift bytes past a 16-byte boundary, the buffer ending with the last of them), outputs
    poisoned, the call -> (status, first_bad, the two output tensors and their leads); nothing is read back"""
    keep, d = [], {}
    for name, a in b.inputs.items():
        t, d[name] = env.dev(a, b.case.shift if name in ("bases", "words") else 0)
        keep.append(t)
    tw, lead_w = env.guarded(np.dtype(np.uint64), b.total)
    tp, lead_p = env.guarded(np.dtype(np.uint8), 4 * b.total)          # bytes of 0xA5: u32 slots of M.POISON_U32
    d["word"], d["pos"] = tw.data_ptr() + 8 * lead_w, tp.data_ptr() + lead_p
    assert d["pos"] % 4 == 0
    st, fb = call(env, b, d)
    return st, fb, (tw, lead_w), (tp, lead_p), keep


def outputs(env, b: M.Built, out_w, out_p, what):
    """the guards are intact -> the interiors (word u64, pos u32)"""
    (tw, lead_w), (tp, lead_p) = out_w, out_p
    hw, hp = env.read(tw), env.read(tp)
    assert (hw[:lead_w] == E.POISON_U64).all() and (hw[lead_w + b.total:] == E.POISON_U64).all(), (what, b.case.id, "guards of d_word")
    assert (hp[:lead_p] == E.POISON_U8).all() and (hp[lead_p + 4 * b.total:] == E.POISON_U8).all(), (what, b.case.id, "guards of d_pos")
    return hw[lead_w: lead_w + b.total], hp[lead_p: lead_p + 4 * b.total].view(np.uint32)


def run(env, b: M.Built, what=""):
    st, fb, out_w, out_p, keep = launch(env, b)
    assert st == b.status, (what, b.case.id, b.n, st)
    if fb is not None:
        assert fb == b.first_bad, (what, b.case.id, b.n, fb)
    word, pos = outputs(env, b, out_w, out_p, what)
    del keep
    if b.status != M.OK:
        return None
    wrong = np.flatnonzero((word != b.word) | (pos != b.pos))
    if len(wrong):
        s = int(wrong[0])
        read, unit, sweep = b.where(s)
        unwritten = int(((word == np.uint64(M.POISON_U64)) & (pos == np.uint32(M.POISON_U32))).sum())
        pytest.fail(f"{what} {b.case.id}: {len(wrong)} of {b.total} slots differ ({unwritten} unwritten); the first is slot {s} of read {read}, "
                    f"unit {unit} = sweep {sweep} (U = {b.U}): word {int(word[s]):#x} pos {int(pos[s])}, expected {int(b.word[s]):#x} {int(b.pos[s])}")
    return word, pos


# ------------------------------------------------------------------ every arm past its cap, and at the edges

@pytest.mark.parametrize("i", range(len(M.CASES)), ids=[c.id for c in M.CASES])
def test_past_one_sweep(env, i):
    """(what the seqvec_slide<M1,k32> case found on the device: DESIGN 4.5)"""
    b = _built(i, n_cu_of(env))
    assert b.units > b.U and b.arm.name in M.ARMS
    run(env, b)


@pytest.mark.parametrize("i", range(len(M.EDGE)), ids=[p.id for p, _ in M.EDGE])
def test_edge_sizes(env, i):
    """1, 15, 16, 17 and U units of one k-mer each (L == k); a single read of 12 bases as the whole batch -- fewer bytes than the
    tiled kernel's prefetch takes from a batch"""
    p, sizes = M.EDGE[i]
    for size in sizes:
        run(env, M.build(p, n_cu_of(env), size), what=size)


@pytest.mark.parametrize("i", range(len(M.BAD)), ids=[p.id for p in M.BAD])
def test_invalid_byte_found_past_the_first_sweep(env, i):
    b = M.build(M.BAD[i], n_cu_of(env), bad=True)
    assert b.status == M.E_INVALID_BASE and b.first_bad >= b.first_past and b.first_bad * b.J >= b.U
    run(env, b)


# ------------------------------------------------------------------ determinism

def test_same_answer_again_and_on_a_side_stream(env):
    """a tiled ragged case twice on the context's stream and once through a fresh context on a stream of its own: identical"""
    import torch

    from kmers_amd.api import Context

    i = next(i for i, c in enumerate(M.CASES) if c.arm.name == "reads_tiled<M1,ragged,k64>")
    b = _built(i, n_cu_of(env))
    first, again = run(env, b, "first"), run(env, b, "again")
    ctx = Context(0, stream=torch.cuda.Stream())
    try:
        side = run(Env(ctx), b, "side stream")
    finally:
        ctx.close()
    for got in (again, side):
        assert E.same(got[0], first[0]) and E.same(got[1], first[1])
