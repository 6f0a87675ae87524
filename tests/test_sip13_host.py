"""CPU-side checks of the *_sip13 calls (SipHash-1-3 under std's DefaultHasher / RandomState): the five symbols are exported and
bound, argument errors come back as the codes of the Lex siblings, the new kernels stay out of scratch, and the numpy SipHash the GPU
tests take their expected values from equals the oracle's."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from tests import sip13_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kmx_canonical_reduce_sip13", "kmx_histogram_sip13", "kmx_minimizer_words_sip13", "kmx_seqvec_minimizers_sip13",
         "kmx_minimizers_sip13"]


@pytest.fixture(scope="module")
def lib():
    from kmers_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def fake_ctx():
    # argument checks run before a call looks at its context: a non-null host address stands in for one (nothing dereferences it
    # on these paths -- a call that got past its checks would need a real GPU context and is never made here)
    buf = C.create_string_buffer(4096)
    return C.cast(buf, C.c_void_p), buf


def test_symbols_exported_and_bound(lib):
    from kmers_amd import _lib

    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert lib.kmx_version() == 2


def _reads(n=4, L=150, bases=0x1000):
    from kmers_amd import _lib

    return _lib.Reads(bases, n, L, None)


def test_reduce_and_histogram_argument_codes(lib, fake_ctx):
    from kmers_amd import _lib

    ctx, _ = fake_ctx
    r = _reads()
    out = C.c_void_p(0x2000)
    for k in (0, 32):
        st = lib.kmx_canonical_reduce_sip13(ctx, C.byref(r), k, 0, 0, 0, out)
        assert st == lib.kmx_canonical_reduce(ctx, C.byref(r), k, _lib.HASH_LEX, k, 0, out) == _lib.E_K_RANGE, k
        st = lib.kmx_histogram_sip13(ctx, C.byref(r), k, 0, 0, 10, out)
        assert st == lib.kmx_histogram(ctx, C.byref(r), k, _lib.HASH_LEX, 31, 10, out) == _lib.E_K_RANGE, k
    assert lib.kmx_histogram_sip13(ctx, C.byref(r), 31, 1, 2, 31, out) == lib.kmx_histogram(ctx, C.byref(r), 31, _lib.HASH_LEX, 31, 31, out) == _lib.E_ARG
    # null pointers: context, reads, output; bases missing for a non-empty batch
    assert lib.kmx_canonical_reduce_sip13(None, C.byref(r), 31, 0, 0, 0, out) == _lib.E_ARG
    assert lib.kmx_canonical_reduce_sip13(ctx, None, 31, 0, 0, 0, out) == _lib.E_ARG
    assert lib.kmx_canonical_reduce_sip13(ctx, C.byref(r), 31, 0, 0, 0, None) == _lib.E_ARG
    assert lib.kmx_histogram_sip13(ctx, C.byref(r), 31, 0, 0, 10, None) == _lib.E_ARG
    nob = _reads(bases=None)
    assert lib.kmx_canonical_reduce_sip13(ctx, C.byref(nob), 31, 0, 0, 0, out) == lib.kmx_canonical_reduce(ctx, C.byref(nob), 31, 0, 0, 0, out) == _lib.E_ARG
    assert lib.kmx_histogram_sip13(ctx, C.byref(nob), 31, 0, 0, 10, out) == _lib.E_ARG


def test_minimizer_argument_codes(lib, fake_ctx):
    from kmers_amd import _lib

    ctx, _ = fake_ctx
    p = C.c_void_p(0x3000)
    # w > k, w = 0, k = 33 for the words call
    for k, w in ((15, 16), (31, 0), (33, 15)):
        st = lib.kmx_minimizer_words_sip13(ctx, p, 10, k, w, 0, 0, p, p)
        assert st == lib.kmx_minimizer_words(ctx, p, 10, k, w, _lib.HASH_IDENTITY, 0, p, p) == _lib.E_K_RANGE, (k, w)
    for k, w in ((15, 16), (31, 0), (40, 33)):
        st = lib.kmx_seqvec_minimizers_sip13(ctx, p, 10, 150, k, w, 0, 0, p, p)
        assert st == lib.kmx_seqvec_minimizers(ctx, p, 10, 150, k, w, _lib.HASH_IDENTITY, 0, p, p) == _lib.E_K_RANGE, (k, w)
        r = _reads()
        st = lib.kmx_minimizers_sip13(ctx, C.byref(r), None, k, w, 0, 0, p, p, None)
        assert st == lib.kmx_minimizers(ctx, C.byref(r), None, k, w, _lib.HASH_IDENTITY, 0, p, p, None) == _lib.E_K_RANGE, (k, w)
    # read_len < k (the iterator asserts sv.len() >= k); null outputs; ragged reads without window offsets
    assert lib.kmx_seqvec_minimizers_sip13(ctx, p, 10, 20, 31, 15, 0, 0, p, p) == _lib.E_ARG
    assert lib.kmx_seqvec_minimizers_sip13(ctx, p, 10, 150, 31, 15, 0, 0, None, p) == _lib.E_ARG
    assert lib.kmx_minimizer_words_sip13(ctx, p, 10, 31, 15, 0, 0, None, p) == _lib.E_ARG
    assert lib.kmx_minimizer_words_sip13(None, p, 10, 31, 15, 0, 0, p, p) == _lib.E_ARG
    short = _reads(L=20)
    assert lib.kmx_minimizers_sip13(ctx, C.byref(short), None, 31, 15, 0, 0, p, p, None) == _lib.E_ARG
    r = _reads()
    assert lib.kmx_minimizers_sip13(ctx, C.byref(r), None, 31, 15, 0, 0, None, p, None) == _lib.E_ARG
    ragged = _lib.Reads(0x1000, 4, 150, 0x4000)
    assert lib.kmx_minimizers_sip13(ctx, C.byref(ragged), None, 31, 15, 0, 0, p, p, None) == _lib.E_ARG
    assert lib.kmx_minimizers_sip13(None, C.byref(r), None, 31, 15, 0, 0, p, p, None) == _lib.E_ARG


def _usage():
    out = {}
    for f in glob.glob(os.path.join(ROOT, "kmers_amd", "csrc", "_obj", "*.usage.txt")):
        for ln in open(f):
            parts = [x.strip() for x in ln.strip().split("|")]
            if len(parts) < 2:
                continue
            out[parts[0]] = {p.rpartition(":")[0].strip(): p.rpartition(":")[2].strip() for p in parts[1:]}
    return out


def test_new_kernels_stay_out_of_scratch():
    kernels = _usage()
    if not kernels:
        pytest.skip("no *.usage.txt next to the objects (library not built by kmers_amd.build in this tree)")
    wanted = ["SinkReduceSip", "SinkHistSip", "reduce_generic_sip_kernel", "histogram_generic_sip_kernel", "minimizers_sip_kernel",
              "minimizer_words_sip_kernel", "SinkHistPartTILi3", "minimizers_sip_generic_kernel"]
    for w in wanted:
        hits = [n for n in kernels if w in n]
        assert hits, f"no kernel built for {w}"
        for n in hits:
            d = kernels[n]
            assert d["Dynamic Stack"] == "False", n
            assert int(d["ScratchSize [bytes/lane]"]) <= 40, (n, d["ScratchSize [bytes/lane]"])


def test_numpy_siphash_equals_the_oracle(orc):
    L = orc.lib()
    rng = np.random.default_rng(13)
    words = rng.integers(0, 2**64, 10_000, dtype=np.uint64)
    words[:4] = [0, 1, 2**64 - 1, 0x0123456789ABCDEF]
    for k0, k1 in ((0, 0), (int(rng.integers(0, 2**63)) * 2 + 1, int(rng.integers(0, 2**64, dtype=np.uint64))), (2**64 - 1, 1), (1, 2**64 - 1)):
        got = sip13_np.siphash13(words, k0, k1)
        want = np.array([L.kmo_siphash13_u64(int(x), k0, k1) for x in words], np.uint64)
        assert (got == want).all(), (k0, k1)


def test_numpy_bucket_function():
    h = np.array([0, 1, 2**64 - 1, 0x9E3779B97F4A7C15], np.uint64)
    for b in (0, 1, 10, 20, 30):
        got = sip13_np.bucket_of(h, b)
        for x, g in zip(h, got):
            x = int(x)
            mix = ((x & 0xFFFFFFFF) * 0x9E3779B1 + (x >> 32) * 0x85EBCA6B) & 0xFFFFFFFF
            assert g == (mix >> (32 - b) if b else 0)
