"""kmx_count_lookup(2) / kmx_count_lookup_reads(2) / kmx_count_spectrum / kmx_count_filter(2) without a GPU: the seven symbols are
exported, bound and declared, argument errors come back as codes (never a crash), and the Rust binding carries the calls."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("kmx_count_lookup", "kmx_count_lookup2", "kmx_count_lookup_reads", "kmx_count_lookup_reads2", "kmx_count_spectrum",
         "kmx_count_filter", "kmx_count_filter2")


def test_query_symbols_are_exported_bound_and_declared():
    from kmers_amd import _lib

    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert f"int {name}(kmx_ctx *ctx," in hdr
    assert "#define KMX_VERSION 2" in hdr and lib.kmx_version() == 2


def test_query_null_ctx_is_an_error_not_a_crash():
    from kmers_amd import _lib

    lib = _lib.load()
    n = C.c_uint64(7)
    r = _lib.Reads(None, 0, 0, None)
    assert lib.kmx_count_lookup(None, None, None, 0, 31, None, None, 0, None) == _lib.E_ARG
    assert lib.kmx_count_lookup2(None, None, None, 0, 47, None, None, 0, None) == _lib.E_ARG
    assert lib.kmx_count_lookup_reads(None, C.byref(r), None, 31, None, None, 0, None) == _lib.E_ARG
    assert lib.kmx_count_lookup_reads(None, None, None, 31, None, None, 0, None) == _lib.E_ARG
    assert lib.kmx_count_lookup_reads2(None, C.byref(r), None, 47, None, None, 0, None) == _lib.E_ARG
    assert lib.kmx_count_spectrum(None, None, 0, 256, None) == _lib.E_ARG
    assert lib.kmx_count_filter(None, None, None, 0, 1, 2, None, None, 0, C.byref(n)) == _lib.E_ARG
    assert lib.kmx_count_filter2(None, None, None, 0, 1, 2, None, None, 0, C.byref(n)) == _lib.E_ARG
    assert lib.kmx_count_filter(None, None, None, 0, 1, 2, None, None, 0, None) == _lib.E_ARG


def test_rust_binding_carries_the_query_calls():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert f"pub fn {name}(" in ffi
        assert f"pub fn {name[4:]}(ctx: &HipContext, " in lib_rs and f"{name}(ctx.0, " in lib_rs


def test_python_api_has_the_query_methods():
    from kmers_amd.api import Context

    for name in NAMES:
        assert callable(getattr(Context, name[4:]))
