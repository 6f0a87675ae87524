"""kmx_count_canonical / kmx_count_merge without a GPU: the symbols are exported and bound, argument errors come back as
codes (never a crash), and the Rust binding is regenerated from the header."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_count_symbols_are_exported_and_bound():
    from kmers_amd import _lib

    lib = _lib.load()
    for name in ("kmx_count_canonical", "kmx_count_merge"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert "int kmx_count_canonical(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k," in hdr
    assert "int kmx_count_merge(kmx_ctx *ctx," in hdr


def test_count_null_ctx_is_an_error_not_a_crash():
    from kmers_amd import _lib

    lib = _lib.load()
    nd = C.c_uint64(7)
    r = _lib.Reads(None, 0, 0, None)
    assert lib.kmx_count_canonical(None, C.byref(r), 31, None, None, 0, C.byref(nd)) == _lib.E_ARG
    assert lib.kmx_count_canonical(None, None, 31, None, None, 0, None) == _lib.E_ARG
    assert lib.kmx_count_merge(None, None, None, 0, None, None, 0, None, None, 0, C.byref(nd)) == _lib.E_ARG


def test_rust_ffi_carries_the_count_calls():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert "pub fn kmx_count_canonical(" in ffi and "pub fn kmx_count_merge(" in ffi
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert "pub fn count_canonical(ctx: &HipContext, d_reads: &DeviceBuf<'_>" in lib_rs
