"""kmx::naive_impl::bgzf_inflate and the BGZF constructor path of kmx::naive_impl::FastqReads (include/kmx.hpp): tests/cpp/test_bgzf_hpp.cpp compiled here
with g++, executed on the GPU over a BGZF image, its text and a plain-gzip image written by this test."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import bgzf_np as B
from tests.fastx_cases import fastq_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_bgzf_hpp.cpp")


def _build(tmp_path):
    lib = os.path.join(ROOT, "kmers_amd", "libkmx.so")
    assert os.path.exists(lib), "build libkmx.so first (python -m kmers_amd.build)"
    exe = str(tmp_path / "test_bgzf_hpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-L", os.path.join(ROOT, "kmers_amd"),
                           "-lkmx", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "kmers_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_cpp_bgzf_compiles(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
def test_cpp_bgzf_on_gpu(tmp_path):
    exe = _build(tmp_path)
    text = fastq_text(np.random.default_rng(21), 400, 30, 150)
    paths = [tmp_path / "r.fastq.gz", tmp_path / "r.fastq", tmp_path / "plain.gz"]
    paths[0].write_bytes(B.write(text, 6, 9000))
    paths[1].write_bytes(text)
    paths[2].write_bytes(gzip.compress(text))
    r = subprocess.run([exe] + [str(p) for p in paths], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all C++ BGZF checks passed" in r.stdout
