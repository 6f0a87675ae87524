"""kmx_count_canonical2 / kmx_count_merge2 (two-word k-mers, k = 33..64) without a GPU: the symbols are exported and bound,
argument errors come back as codes (never a crash), the header documents the working set the layout was built for, and the Rust
binding carries the calls."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_count2_symbols_are_exported_and_bound():
    from kmers_amd import _lib

    lib = _lib.load()
    for name in ("kmx_count_canonical2", "kmx_count_merge2"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert _lib.SIGNATURES["kmx_count_canonical2"] == _lib.SIGNATURES["kmx_count_canonical"]
    assert _lib.SIGNATURES["kmx_count_merge2"] == _lib.SIGNATURES["kmx_count_merge"]
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    assert "int kmx_count_canonical2(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, uint64_t *d_kmers2, uint64_t *d_counts," in hdr
    assert "int kmx_count_merge2(kmx_ctx *ctx, const uint64_t *d_kmers2_a," in hdr
    assert "at most 36 bytes per window" in hdr and "24 bytes per input entry" in hdr
    assert "#define KMX_VERSION 2\n" in hdr


def test_count2_null_arguments_are_errors_not_crashes():
    from kmers_amd import _lib

    lib = _lib.load()
    nd = C.c_uint64(7)
    r = _lib.Reads(None, 0, 0, None)
    for k in (32, 33, 47, 64, 65):      # (a NULL context is an argument error whatever k is)
        assert lib.kmx_count_canonical2(None, C.byref(r), k, None, None, 0, C.byref(nd)) == _lib.E_ARG
    assert lib.kmx_count_canonical2(None, None, 47, None, None, 0, C.byref(nd)) == _lib.E_ARG
    assert lib.kmx_count_canonical2(None, None, 47, None, None, 0, None) == _lib.E_ARG
    assert lib.kmx_count_merge2(None, None, None, 0, None, None, 0, None, None, 0, C.byref(nd)) == _lib.E_ARG
    assert lib.kmx_count_merge2(None, None, None, 0, None, None, 0, None, None, 0, None) == _lib.E_ARG
    assert nd.value == 7                # nothing was written through the pointer


def test_api_has_the_two_word_methods():
    import inspect

    from kmers_amd.api import Context

    one = inspect.signature(Context.count_canonical)
    two = inspect.signature(Context.count_canonical2)
    assert list(one.parameters) == list(two.parameters)
    assert list(inspect.signature(Context.count_merge).parameters) == list(inspect.signature(Context.count_merge2).parameters)


def test_rust_binding_carries_the_two_word_count_calls():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert "pub fn kmx_count_canonical2(" in ffi and "pub fn kmx_count_merge2(" in ffi
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert "pub fn count_canonical2(ctx: &HipContext, d_reads: &DeviceBuf<'_>" in lib_rs
    assert "pub fn count_merge2(ctx: &HipContext" in lib_rs
    assert "kmx_count_canonical2(ctx.0" in lib_rs and "kmx_count_merge2(ctx.0" in lib_rs
