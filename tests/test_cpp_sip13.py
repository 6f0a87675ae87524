"""include/kmx.hpp's SipHasher13State overloads (canonical_reduce, Kmer::minimizer, SeqVector::iter_minimizers), built with g++ the
way test_cpp_host_layer.py builds its binary and run on the GPU: the same results as the Python path on a small batch, and the
kmer.rs:560-580 property of Kmer::minimizer."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_sip13_hpp.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_sip13_hpp")
KEY = (0x0706050403020100, 0x0F0E0D0C0B0A0908)


def _build():
    lib = os.path.join(ROOT, "kmers_amd", "libkmx.so")
    assert os.path.exists(lib), "build libkmx.so first (python -m kmers_amd.build)"
    deps = [SRC, os.path.join(ROOT, "include", "kmx.hpp"), os.path.join(ROOT, "include", "kmx.h"), lib]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC,
                               "-L", os.path.join(ROOT, "kmers_amd"), "-lkmx", "-L/opt/rocm/lib",
                               "-Wl,-rpath," + os.path.join(ROOT, "kmers_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", EXE])
    return EXE


def _batch(nbytes):
    out = np.empty(nbytes, np.uint8)
    x = 12345
    for i in range(nbytes):
        x = (x * 6364136223846793005 + 1442695040888963407) & (2**64 - 1)
        out[i] = b"ACGT"[(x >> 33) & 3]
    return out


@pytest.mark.gpu
def test_cpp_sip13_overloads_match_the_python_path():
    exe = _build()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all sip13 C++ checks passed" in r.stdout
    from kmers_amd.api import Context

    ctx = Context()
    try:
        n, L = 70, 150
        host = _batch(n * L)
        dev = ctx.to_device(host)
        lines = r.stdout.splitlines()
        for fl in (0, 1):
            g = ctx.canonical_reduce_sip13(dev, n, L, 31, *KEY, flags=fl)
            assert f"reduce {fl} {g.n_valid} {g.sum_canon} {g.xor_hash} {g.sum_fw}" in lines
        sv = ctx.seqvec_from_bytes(ctx.to_device(host[:L]))
        mw, mp = ctx.seqvec_minimizers_sip13(sv, 1, L, 31, 15, *KEY)
        want = [f"mm {a} {b}" for a, b in zip(mw.cpu().numpy().view(np.uint64), mp.cpu().numpy())]
        assert [ln for ln in lines if ln.startswith("mm ")] == want
        words = ctx.kmers_from_bytes(ctx.to_device(np.concatenate([host[i * 7: i * 7 + 31] for i in range(20)])), 20, 31)
        mm, off = ctx.minimizer_words_sip13(words, 31, 15, *KEY)
        want = [f"kmer {i} {a} {b}" for i, (a, b) in enumerate(zip(mm.cpu().numpy().view(np.uint64), off.cpu().numpy()))]
        assert [ln for ln in lines if ln.startswith("kmer ")] == want
    finally:
        ctx.close()
