"""The host model of the distinct-key estimator (tests/hll_np.py) pinned without a GPU, and the host sides that must agree with it.

* Accuracy: the model's estimate against the exact distinct count of fixed-seed random keys.  The allowed relative error is
  hll_np.tolerance(p) = 4 * 1.04 / sqrt(2^p), four times the estimator's asymptotic standard error: a condition, not a measurement.
  The seeds below are fixed; the model alone stays inside it on them (p = 4 does not promise that and is used for bytes only).
* Laws: n = 0 gives 0, few keys in many registers are counted almost exactly, registers(a u b) == max(registers(a), registers(b)),
  adding keys again changes nothing, inv_fmix64 inverts fmix64, and placed keys land where they were placed.
* Host agreement: kmers_amd.api.hll_estimate equals the model's estimate on the same bins to 1e-12 relative, and
  hll_sketch_log2_blocks the closed form.
* Declarations: header, ffi.rs, kmx.hpp, lib.rs and _lib.SIGNATURES declare every new name; the source is built and the key hash has
  one definition."""
import math
import os
import re

import numpy as np
import pytest

from tests import hll_np as hl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kmx_hll_add_words", "kmx_hll_add_words2", "kmx_hll_add", "kmx_hll_add2", "kmx_hll_merge", "kmx_hll_stats")


def _distinct_keys(rng, n, words=1):
    a = rng.integers(0, 2**64, (n, words), dtype=np.uint64)
    if words == 1:
        return np.unique(a[:, 0])
    return np.unique(a, axis=0)


@pytest.mark.parametrize("p", (9, 12, 14, 18))
@pytest.mark.parametrize("n", (0, 1, 100, 10_000, 300_000, 1_000_000))
def test_estimate_within_four_standard_errors(p, n):
    rng = np.random.default_rng(1000 * p + n % 997)
    keys = _distinct_keys(rng, n)
    regs = hl.registers(keys, p, seed=p)
    est = hl.estimate(hl.bins(regs), p)
    print(f"p={p} n={len(keys)} estimate={est:.1f}")
    if len(keys) == 0:
        assert est == 0.0
    else:
        assert abs(est - len(keys)) / len(keys) <= hl.tolerance(p)


def test_two_word_keys_estimate():
    rng = np.random.default_rng(5)
    keys = _distinct_keys(rng, 200_000, 2)
    est = hl.estimate(hl.bins(hl.registers(keys, 14, seed=1)), 14)
    assert abs(est - len(keys)) / len(keys) <= hl.tolerance(14)
    # the hash reads both words: the low words alone are another set of registers
    assert (hl.registers(keys, 14, seed=1) != hl.registers(keys[:, 0], 14, seed=1)).any()


def test_simple_laws():
    rng = np.random.default_rng(8)
    for p in (4, 9, 14, 24):
        assert hl.estimate(hl.bins(np.zeros(1 << p, np.uint8)), p) == 0.0
    keys = _distinct_keys(rng, 1000)
    for p in (18, 20):                                                    # n much smaller than m: almost exact
        est = hl.estimate(hl.bins(hl.registers(keys, p)), p)
        assert abs(est - len(keys)) / len(keys) < 0.01
    a, b = _distinct_keys(rng, 30_000), _distinct_keys(rng, 50_000)
    b[:10_000] = a[:10_000]                                               # an overlap
    for p in (4, 12):
        ra, rb = hl.registers(a, p, seed=3), hl.registers(b, p, seed=3)
        whole = hl.registers(np.concatenate([a, b]), p, seed=3)
        assert (hl.merge(ra, rb) == whole).all() and (hl.merge(rb, ra) == whole).all()
        assert (hl.registers(a, p, seed=3, into=whole) == whole).all()    # idempotent
        assert (hl.registers(b, p, seed=3, into=ra) == whole).all()       # accumulation == union
        assert int(hl.bins(whole).sum()) == 1 << p
    flags = (rng.random(len(a)) < 0.5).astype(np.uint8) * 3
    assert (hl.registers(a, 9, flags=flags) == hl.registers(a[flags != 0], 9)).all()


def test_inverse_hash_places_keys():
    rng = np.random.default_rng(2)
    x = rng.integers(0, 2**64, 1000, dtype=np.uint64)
    assert (hl.inv_fmix64(hl.fmix64(x)) == x).all() and (hl.fmix64(hl.inv_fmix64(x)) == x).all()
    for seed in (0, 7, 2**64 - 1):
        assert (hl.key_hash(hl.keys_for_hashes(x, seed), seed) == x).all()
    for p in (4, 14):
        q = 64 - p
        # one key per register with rank 1: the bit below the index set
        h = (np.arange(1 << p, dtype=np.uint64) << np.uint64(q)) | np.uint64(1 << (q - 1))
        idx, rank = hl.idx_rank(h, p)
        assert (idx == np.arange(1 << p)).all() and (rank == 1).all()
        # every rank 1 .. 65 - p in register 3: a single bit at q - r, and w == 0
        h = np.array([(3 << q) | (1 << (q - r)) for r in range(1, q + 1)] + [3 << q], np.uint64)
        idx, rank = hl.idx_rank(h, p)
        assert (idx == 3).all() and [int(r) for r in rank] == list(range(1, q + 2))
        regs = hl.registers(hl.keys_for_hashes(h, 5), p, seed=5)
        assert regs[3] == q + 1 == 65 - p and np.count_nonzero(regs) == 1


def test_known_answers():
    # worked out with plain Python integers from the definition in include/kmx.h: key 0 under seed 0 hashes to 0x6393D51C06C618DC
    h = 0x6393D51C06C618DC
    assert int(hl.key_hash(np.zeros(1, np.uint64), 0)[0]) == h
    for p in (4, 14, 24):
        w = (h << p) & (2**64 - 1)
        idx, rank = hl.idx_rank(np.array([h], np.uint64), p)
        assert int(idx[0]) == h >> (64 - p) and int(rank[0]) == min(64 - w.bit_length(), 64 - p) + 1


def test_host_estimate_agrees_with_the_model():
    from kmers_amd.api import hll_estimate, hll_sketch_log2_blocks

    rng = np.random.default_rng(12)
    for p, n in ((4, 50), (9, 0), (9, 700), (12, 100_000), (14, 3), (14, 200_000), (18, 1_000_000)):
        hist = hl.bins(hl.registers(_distinct_keys(rng, n), p))
        want, got = hl.estimate(hist, p), hll_estimate(hist, p)
        assert got == want or abs(got - want) <= 1e-12 * want, (p, n, got, want)
        assert hll_estimate([int(v) for v in hist], p) == got            # a list of ints is taken too
    # every register one below the top rank: only the chain is left, z = m / 2^q ...
    hist = np.zeros(64, np.uint64)
    hist[64 - 14] = 1 << 14
    assert hll_estimate(hist, 14) == hl.estimate(hist, 14) == 2.0**14 * 2.0**50 / (2.0 * math.log(2.0))
    # ... and every register at the top rank: tau(0) = 0 and sigma(0) = 0 leave z = 0, no upper end
    hist[64 - 14], hist[65 - 14] = 0, 1 << 14
    assert hll_estimate(hist, 14) == hl.estimate(hist, 14) == math.inf
    with pytest.raises(ValueError):
        hll_estimate(hist, 3)
    with pytest.raises(ValueError):
        hll_estimate(hist, 13)                                            # the bins of another size
    for e in (0.0, 1.0, 4.0, 5.0, 1e3, 3.3e5, 1e6, 7.7e8, 1e10, 1e13):
        for fill in (0.25, 0.5, 0.1):
            b = hll_sketch_log2_blocks(e, fill)
            assert b == hl.sketch_log2_blocks(e, fill), (e, fill)
            assert b == 32 or 1.0 - math.exp(-e / (16.0 * 2.0**b)) <= fill
            assert b == 0 or 1.0 - math.exp(-e / (16.0 * 2.0**(b - 1))) > fill
    # DESIGN's "about 14 bytes per distinct k-mer" at a quarter full: 64 / (16 * -ln 0.75) = 13.9, up to twice that with the
    # rounding up to a power of two
    for e in (1e6, 3e7, 2e9):
        assert 13.9 <= (64 << hll_sketch_log2_blocks(e)) / e < 27.9
    with pytest.raises(ValueError):
        hll_sketch_log2_blocks(1e6, 1.0)


def test_cpp_estimate_agrees_with_the_model(tmp_path):
    """kmx::hll_estimate of include/kmx.hpp, compiled here with the host compiler, on the model's bins"""
    import shutil
    import subprocess

    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    lib = os.path.join(ROOT, "kmers_amd", "libkmx.so")
    if not cxx:
        pytest.skip("no host C++ compiler")
    assert os.path.exists(lib), "build libkmx.so first (python -m kmers_amd.build)"
    exe = str(tmp_path / "hll_estimate_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "hll_estimate_check.cpp"),
                           "-L", os.path.join(ROOT, "kmers_amd"), "-lkmx", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "kmers_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    rng = np.random.default_rng(13)
    for p, n in ((4, 50), (9, 0), (12, 100_000), (14, 200_000), (24, 1000)):
        hist = hl.bins(hl.registers(_distinct_keys(rng, n), p))
        r = subprocess.run([exe, str(p)] + [str(int(v)) for v in hist], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got, b = r.stdout.split()
        want = hl.estimate(hist, p)
        assert float(got) == want or abs(float(got) - want) <= 1e-12 * want, (p, n, got, want)
        assert int(b) == hl.sketch_log2_blocks(want)


def test_calls_declared_bound_built_and_in_rust():
    from kmers_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    hpp = open(os.path.join(ROOT, "include", "kmx.hpp")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.SIGNATURES and re.search(r"pub fn %s\b" % name, ffi), name
        assert re.search(r"\b%s\s*\(" % name, hpp) and re.search(r"\b%s\s*\(" % name, rs), name
    assert "class Hll" in hpp and re.search(r"\bhll_estimate\s*\(", hpp) and re.search(r"pub fn hll_estimate\b", rs)
    assert "kmx_hll.hip" in build.SOURCES
    for src in ("kmx_hll.hip", "kmx_sketch.hip"):
        names = [os.path.basename(h) for h in build._headers_of(src)]
        assert "kmx_key_hash.h" in names and "kmx_count_common.h" in names
    assert not any(os.path.basename(h) == "kmx_key_hash.h" for h in build._headers_of("kmx_count.hip"))
    # one definition of the key hash: in the header both sources include, in neither of them
    csrc = os.path.join(ROOT, "kmers_amd", "csrc")
    assert len(re.findall(r"u64 key_hash<1>", open(os.path.join(csrc, "kmx_key_hash.h")).read())) == 1
    for src in ("kmx_hll.hip", "kmx_sketch.hip"):
        txt = open(os.path.join(csrc, src)).read()
        assert '#include "kmx_key_hash.h"' in txt and "u64 key_hash<" not in txt and "0x9E3779B97F4A7C15" not in txt
    assert _lib.HLL_MIN_LOG2_REGS == 4 and _lib.HLL_MAX_LOG2_REGS == 24 and _lib.HLL_BINS == 64
    assert re.search(r"HLL_LDS_MAX_LOG2_REGS = %d;" % _lib.HLL_LDS_MAX_LOG2_REGS, open(os.path.join(csrc, "kmx_hll.hip")).read())
    assert re.search(r"HLL_LDS_KEYS_PER_DWORD = %d;" % _lib.HLL_LDS_KEYS_PER_DWORD, open(os.path.join(csrc, "kmx_hll.hip")).read())


def test_null_context_is_an_argument_error():
    from kmers_amd import _lib

    lib = _lib.load()
    assert lib.kmx_hll_add_words(None, None, 0, None, 14, 0) == _lib.E_ARG
    assert lib.kmx_hll_add(None, None, 31, None, 14, 0) == _lib.E_ARG
    assert lib.kmx_hll_merge(None, None, None, 14, None) == _lib.E_ARG
    assert lib.kmx_hll_stats(None, None, None, 14, None) == _lib.E_ARG
