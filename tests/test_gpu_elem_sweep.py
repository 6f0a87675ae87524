"""The one-element-per-lane calls (kmx_elem.hip, the first half of kmx_seqvec.hip) past one grid sweep.

Every kernel of the family is a grid-stride loop behind a grid capped at 16 * n_cu blocks of 256 threads (8 * n_cu for the two offset
kernels).  S = 16 * n_cu * 256 is read from the device; the `past` size class gives a launch S + S // 3 + 1 work items, so some threads
take two iterations, some one, and the last block is partial; the edge class is n in {0, 1, 2, 3, 255, 256, 257}.

All calls go through the C ABI (the wrappers allocate aligned outputs of their own and cannot alias).  Every output is the interior of
a larger poisoned tensor -- 16 u64 or 128 bytes of guard on either side -- and after the call the guards are intact and the interior
equals tests/elem_np.py's numpy reference, exactly.  The inputs, the references and the proof that these cases could not pass with a
kernel that stops after one sweep are in tests/elem_np.py and tests/test_elem_np.py (CPU).

Aliasing: d_out == d_in is allowed (and documented in include/kmx.h) for kmx_revcomp_words, kmx_canonical_words, kmx_hash_words,
kmx_hash_words_sip13, kmx_sub_kmer_words and kmx_encoding_rev_comp: every lane reads its own elements before it writes them.  Two of
the conditions on in-place inputs cannot be met by construction and are replaced in test_elem_np.py: the identity hasher's output is
its input, and kmx_canonical_words changes only the words of the non-canonical strand (a quarter to three quarters of them)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import elem_np as E

pytestmark = pytest.mark.gpu

IDS = E.case_ids()
M64 = E.M64


class Env:
    def __init__(self, ctx):
        import torch

        self.torch, self.ctx, self.lib, self.h = torch, ctx, ctx.lib, ctx._h
        self.S = 16 * torch.cuda.get_device_properties(ctx.device).multi_processor_count * 256

    def dev(self, a, shift=0):
        """`a` on the device, its first byte `shift` bytes past a 16-byte boundary -> (tensor kept alive, address)"""
        lead = shift // a.itemsize
        t = self.ctx.to_device(np.concatenate([np.zeros(lead, a.dtype), a]) if lead else a)
        assert t.data_ptr() % 16 == 0
        return t, t.data_ptr() + lead * a.itemsize

    def guarded(self, dtype, n, init=None, shift=0):
        """a poisoned buffer with n elements (holding `init`, if given) between its guards -> (tensor, elements before the interior)"""
        u = dtype == np.uint64
        guard, fill = (E.GUARD_WORDS, E.POISON_U64) if u else (E.GUARD_BYTES, E.POISON_U8)
        lead = guard + shift // (8 if u else 1)
        host = np.full(lead + n + guard, fill, dtype)
        if init is not None:
            host[lead:lead + n] = init
        t = self.ctx.to_device(host)
        assert t.data_ptr() % 16 == 0
        return t, lead

    def read(self, t):
        # as the fuzz files read: the current stream waits for the context's, no host synchronisation
        self.torch.cuda.current_stream(self.ctx.device).wait_stream(self.ctx.stream)
        a = t.cpu().numpy()
        return a.view(np.uint64) if a.dtype == np.int64 else a


@pytest.fixture(scope="module")
def env():
    from kmers_amd.api import Context

    ctx = Context(0)
    yield Env(ctx)
    ctx.close()


@functools.lru_cache(maxsize=2)
def _case(S, op, i, size, even=False):
    return E.build(op, E.OPS[op][i], S, size, even=even)


def _vp(x):
    return C.c_void_p(x) if x else None


def call(env, c, d):
    """the C ABI call of case c on the device addresses d -> (status, *h_first_bad or None)"""
    from kmers_amd import _lib

    L, h, p, n, op = env.lib, env.h, c.params, c.n, c.op
    g = lambda name: _vp(d.get(name))
    fb = C.c_uint64(0x1234)
    if op == "kmers_from_bytes":
        return L.kmx_kmers_from_bytes(h, g("seqs"), n, p["k"], g("out"), C.byref(fb)), fb.value
    if op == "revcomp_words":
        return L.kmx_revcomp_words(h, g("in"), n, p["k"], g("out")), None
    if op == "canonical_words":
        return L.kmx_canonical_words(h, g("in"), n, p["k"], g("out"), g("flags")), None
    if op == "hash_words":
        return L.kmx_hash_words(h, g("in"), n, p["hasher"], p["hk"], g("out")), None
    if op == "hash_words_sip13":
        return L.kmx_hash_words_sip13(h, g("in"), n, p["k0"], p["k1"], g("out")), None
    if op == "match_words":
        return L.kmx_match_words(h, g("fw"), g("rc"), g("other"), n, g("out")), None
    if op == "ck_shift":
        fn = L.kmx_ck_append_bases if p["append"] else L.kmx_ck_prepend_bases
        return fn(h, g("fw"), g("rc"), g("bases"), n, p["k"], g("dropped")), None
    if op == "sub_kmer_words":
        return L.kmx_sub_kmer_words(h, g("in"), n, p["k"], p["pos"], p["width"], g("out")), None
    if op == "kmers_to_strings":
        return L.kmx_kmers_to_strings(h, g("in"), n, p["k"], g("out")), None
    if op == "bitmers_to_bytes":
        return L.kmx_bitmers_to_bytes(h, g("in"), n, p["k"], g("out")), None
    enc = E.ENCS.get(p.get("enc"))
    if op == "encode_kmers":
        return L.kmx_encode_kmers(h, g("seqs"), n, p["seq_len"], enc, p["B"], g("out")), None
    if op == "encoding_rev_comp":
        return L.kmx_encoding_rev_comp(h, g("in"), n, p["K"], enc, p["B"], g("out")), None
    if op == "encoding_decode":
        return L.kmx_encoding_decode(h, g("in"), n, enc, p["B"], g("out")), None
    if op == "encode_windows":
        r = _lib.Reads(g("bases") if n else None, n, p["L"], None)
        return L.kmx_encode_windows(h, C.byref(r), p["k"], enc, p["B"], g("out")), None
    if op in ("encode_kmers_p", "encoding_rev_comp_p", "encoding_decode_p"):
        nb = p["bits"] // 8 * p["B"]
        if op == "encode_kmers_p":
            return L.kmx_encode_kmers_p(h, g("seqs"), n, 4 * nb - 1, enc, p["bits"], p["B"], g("out")), None
        if op == "encoding_rev_comp_p":
            return L.kmx_encoding_rev_comp_p(h, g("in"), n, 4 * nb - 1, enc, p["bits"], p["B"], g("out")), None
        return L.kmx_encoding_decode_p(h, g("in"), n, enc, p["bits"], p["B"], g("out")), None
    if op == "seqvec_push_chars":
        # the vector starts n_before // 32 words before the first word that receives bases: those words are guards too
        return L.kmx_seqvec_push_chars(h, _vp(d["words"] - 8 * (p["n_before"] // 32)), p["n_before"], g("bytes"), n, C.byref(fb)), fb.value
    if op == "seqvec_to_bytes":
        return L.kmx_seqvec_to_bytes(h, g("words"), n, g("out")), None
    if op == "seqvec_get_kmers":
        return L.kmx_seqvec_get_kmers(h, g("words"), p["n_bases"], g("pos"), n, p["k"], g("out")), None
    if op == "seqvec_iter_kmers":
        return L.kmx_seqvec_iter_kmers(h, g("words"), p["n_bases"], p["start"], p["end"], p["k"], g("out")), None
    if op == "gen_reads":
        return L.kmx_gen_reads(h, p["seed"], p["first_byte"], g("out"), n), None
    raise KeyError(op)


def run(env, c, in_shift=0, out_shift=0, alias=False, what=""):
    """Run case c with its outputs between guards.  in_shift / out_shift: bytes past a 16-byte boundary of the map_words input / of
    the output "out" (past a 4-byte boundary for the byte outputs).  alias: the call gets ONE array as c.alias's input and output."""
    keep, d, outs = [], {}, {}
    for name, a in c.inputs.items():
        if alias and name == c.alias[0]:
            continue
        t, d[name] = env.dev(a, in_shift if name == c.vec else 0)
        keep.append(t)
    for name, exp in c.outputs.items():
        init = c.inputs[c.alias[0]] if alias and name == c.alias[1] else c.init.get(name)
        t, lead = env.guarded(exp.dtype, len(exp), init, out_shift if name == "out" else 0)
        outs[name] = (t, lead)
        d[name] = t.data_ptr() + lead * exp.itemsize
    if alias:
        d[c.alias[0]] = d[c.alias[1]]
    st, fb = call(env, c, d)
    assert st == c.status, (what, c.op, c.params, c.n, st)
    if c.first_bad is not None:
        assert fb == c.first_bad, (what, c.op, c.params, c.n, fb)
    for name, exp in c.outputs.items():
        t, lead = outs[name]
        host = env.read(t)
        fill = E.POISON_U64 if host.dtype == np.uint64 else E.POISON_U8
        assert (host[:lead] == fill).all() and (host[lead + len(exp):] == fill).all(), (what, c.op, c.params, c.n, name, "guards")
        if c.status == E.OK:       # (after an error the outputs are unspecified)
            got = host[lead:lead + len(exp)]
            assert E.same(got, exp), (what, c.op, c.params, c.n, name, int(np.flatnonzero(got != exp)[0]) if got.shape == exp.shape else got.shape)


# ------------------------------------------------------------------ every call, past the cap and at the edges

@pytest.mark.parametrize("op,i", IDS, ids=[E.case_name(*c) for c in IDS])
def test_past_one_sweep(env, op, i):
    c = _case(env.S, op, i, "past")
    assert c.items > env.S
    run(env, c)


@pytest.mark.parametrize("op,i", IDS, ids=[E.case_name(*c) for c in IDS])
def test_edge_sizes(env, op, i):
    for n in E.EDGE:                # n = 0: KMX_OK and nothing touched (the whole buffer is guard)
        run(env, E.build(op, E.OPS[op][i], env.S, n))


# ------------------------------------------------------------------ alignment

MAPS = [("revcomp_words", 2), ("canonical_words", 4), ("hash_words", 1), ("hash_words", 3), ("hash_words_sip13", 1)]


@pytest.mark.parametrize("op,i", MAPS, ids=[E.case_name(*c) for c in MAPS])
def test_map_words_alignment(env, op, i):
    """the 16-byte pairs with and without the scalar tail, and the scalar fallback when either array is 8 bytes off"""
    assert op in E.MAP_WORDS and E.OPS[op][i].get("form", "words") == "words"
    for size, even in (("past", False), ("past", True), (257, False), (256, False)):
        c = _case(env.S, op, i, size, even)
        assert c.n % 2 == (0 if even or size == 256 else 1)
        for in_shift, out_shift in ((0, 0), (8, 0), (0, 8), (8, 8)):
            run(env, c, in_shift, out_shift, what=(in_shift, out_shift))


BYTE_OUT = [(op, i) for op in ("kmers_to_strings", "bitmers_to_bytes") for i in range(6)] + [("encoding_decode_p", i) for i in range(3)]


@pytest.mark.parametrize("op,i", BYTE_OUT, ids=[E.case_name(*c) for c in BYTE_OUT])
def test_byte_output_alignment(env, op, i):
    """dword or byte stores by the address modulo 4: every start, so that every mix of the two occurs"""
    for size in ("past", 257):
        c = _case(env.S, op, i, size)
        for shift in range(4):
            run(env, c, out_shift=shift, what=shift)


def test_gen_reads_misaligned_output_takes_the_byte_path(env):
    i = [p["path"] for p in E.OPS["gen_reads"]].index("vec")
    c = _case(env.S, "gen_reads", i, "past")
    assert c.params["first_byte"] % 16 == 0
    run(env, c, out_shift=1)
    run(env, E.build("gen_reads", E.OPS["gen_reads"][i], env.S, 257), out_shift=1)


# ------------------------------------------------------------------ aliasing: d_out == d_in

def _find(op, **kw):
    return next(i for i, p in enumerate(E.OPS[op]) if all(p[k] == v for k, v in kw.items()))


ALIAS = [("revcomp_words", _find("revcomp_words", k=31)), ("canonical_words", _find("canonical_words", k=31, form="words")),
         ("canonical_words", _find("canonical_words", k=16, form="both")), ("hash_words", _find("hash_words", hk=20)),
         ("hash_words", _find("hash_words", hasher=E.HASH_IDENTITY)), ("hash_words_sip13", 1), ("sub_kmer_words", 0),
         ("encoding_rev_comp", _find("encoding_rev_comp", enc="ACGT", K=31, B=1)), ("encoding_rev_comp", _find("encoding_rev_comp", enc="ACTG", K=33, B=2))]


@pytest.mark.parametrize("op,i", ALIAS, ids=[E.case_name(*c) for c in ALIAS])
def test_in_place(env, op, i):
    """d_out == d_in exactly, 16-byte aligned and 8 bytes off (the identity hasher is exempt from "the output differs from the
    input": its output is its input -- what it shows in place is that nothing else is disturbed)"""
    for size in ("past", 257):
        c = _case(env.S, op, i, size)
        assert c.alias == ("in", "out")
        for shift in (0, 8):
            run(env, c, out_shift=shift, alias=True, what=("in place", shift))


def test_rev_comp_p_still_rejects_in_place(env):
    c = E.build("encoding_rev_comp_p", E.OPS["encoding_rev_comp_p"][0], env.S, 257)
    t, at = env.dev(c.inputs["in"])
    assert call(env, c, {"in": at, "out": at})[0] == E.E_ARG
    assert E.same(env.read(t), c.inputs["in"])


def test_side_stream_chain_in_place():
    """a second context on a stream of its own: hash_words_sip13, then revcomp_words in place on its output, read on the default
    stream after wait_stream"""
    import torch

    from kmers_amd.api import Context
    from tests import sip13_np

    ctx = Context(0, stream=torch.cuda.Stream())
    try:
        env = Env(ctx)
        c = _case(env.S, "hash_words_sip13", 1, "past")
        p = c.params
        src, at_in = env.dev(c.inputs["in"])
        buf, lead = env.guarded(np.dtype(np.uint64), c.n)
        at = buf.data_ptr() + 8 * lead
        assert env.lib.kmx_hash_words_sip13(env.h, C.c_void_p(at_in), c.n, p["k0"], p["k1"], C.c_void_p(at)) == E.OK
        assert env.lib.kmx_revcomp_words(env.h, C.c_void_p(at), c.n, 32, C.c_void_p(at)) == E.OK
        host = env.read(buf)
        assert E.same(host[lead:lead + c.n], E.revcomp_word(sip13_np.siphash13(c.inputs["in"], p["k0"], p["k1"]), 32))
        assert (host[:lead] == E.POISON_U64).all() and (host[lead + c.n:] == E.POISON_U64).all()
        del src
    finally:
        ctx.close()


# ------------------------------------------------------------------ errors found in the second sweep

def test_first_bad_base_past_the_cap(env):
    S = env.S
    for op, p, per in (("kmers_from_bytes", dict(k=31), 31), ("seqvec_push_chars", dict(n_before=5), 32)):
        lo, hi = (S + 11) * per + 3, (S + S // 4) * per
        c = E.build(op, p, S, "past", bad=(hi, lo))
        assert c.status == E.E_INVALID_BASE and c.first_bad == lo
        run(env, c)


def test_position_outside_the_vector_past_the_cap(env):
    c = E.build("seqvec_get_kmers", dict(k=31), env.S, "past", bad=(env.S + 5,))
    assert c.status == E.E_ARG
    run(env, c)


# ------------------------------------------------------------------ the two 8 * n_cu kernels

@pytest.mark.parametrize("where", ["second", "last"])
def test_length_range_decided_in_the_second_sweep(env, where):
    off, mn, mx, (lo, hi) = E.length_range_offsets(env.S // 2, where)
    assert min(lo, hi) >= env.S // 2
    assert env.ctx.reads_length_range(env.ctx.to_device(off)) == (mn, mx)


@pytest.fixture(scope="module")
def gate_batch(env, orc):
    """bases of the gate batches (one random stream; the offsets alone say which read is short) and the oracle's summaries"""
    S8 = env.S // 2
    n = E.gate_reads(S8)
    bases = E.gen_reads(21, 0, n * E.GATE_L)
    want = {}
    for where in ("second", "last", "tail", "none"):
        off = E.gate_offsets(S8, where)
        o = orc.canonical_reduce(bases[: int(off[-1])], n, 0, E.GATE_K, hasher_k=E.GATE_K, offsets=off)
        want[where] = (o.n_valid, o.sum_canon, o.xor_hash)
    return env.ctx.to_device(bases), n, want


@pytest.mark.parametrize("where", ["second", "last", "tail", "none"])
def test_uniform_gate_decided_past_one_sweep(env, gate_batch, where):
    """kmx_canonical_reduce behind offsets: reads of 33 bases, one of them 32 -- found by the first offset pair of the gate's second
    sweep, by its last pair, by the odd tail offset -- or none: the whole batch against the oracle, with the bound given and without"""
    from kmers_amd import _lib

    d_bases, n, want = gate_batch
    S8 = env.S // 2
    assert (n + 1) % 2 == 1 and (n + 1) // 2 > S8
    d_off = env.ctx.to_device(E.gate_offsets(S8, where))
    for read_len in (E.GATE_L, 0):
        g = env.ctx.canonical_reduce(d_bases, n, read_len, E.GATE_K, _lib.HASH_LEX, E.GATE_K, 0, offsets=d_off)
        assert (g.n_valid, g.sum_canon, g.xor_hash) == want[where], (where, read_len)
    assert want[where][0] == n * (E.GATE_L - E.GATE_K + 1) - (0 if where == "none" else 1)
