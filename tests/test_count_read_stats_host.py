"""kmx_count_read_stats(2) without a GPU: the two symbols are exported, bound and declared, the KMX_RS_* indices of the header are
those of the Python binding, argument errors come back as codes (never a crash), the Rust binding carries the calls, and
read_stats_span decodes a row."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("kmx_count_read_stats", "kmx_count_read_stats2")
FIELDS = ("N_VALID", "N_PRESENT", "N_SOLID", "MIN", "MAX", "SUM", "MEDIAN", "SPAN")


def test_read_stats_symbols_are_exported_bound_and_declared():
    from kmers_amd import _lib

    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert f"int {name}(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k," in hdr
    assert _lib.SIGNATURES[NAMES[0]] == _lib.SIGNATURES[NAMES[1]]
    assert "#define KMX_VERSION 2" in hdr and lib.kmx_version() == 2


def test_read_stats_indices_of_the_header_are_those_of_the_binding():
    from kmers_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+KMX_RS_([A-Z_]+)\s+(\d+)u?\b", hdr, flags=re.M)}
    assert defs.pop("WORDS") == _lib.RS_WORDS == 8
    assert sorted(defs) == sorted(FIELDS)
    for i, f in enumerate(FIELDS):
        assert defs[f] == getattr(_lib, "RS_" + f) == i


def test_read_stats_null_arguments_are_errors_not_crashes():
    from kmers_amd import _lib

    lib = _lib.load()
    r = _lib.Reads(None, 0, 0, None)
    assert lib.kmx_count_read_stats(None, C.byref(r), 31, None, None, 0, 2, None) == _lib.E_ARG
    assert lib.kmx_count_read_stats(None, None, 31, None, None, 0, 2, None) == _lib.E_ARG
    assert lib.kmx_count_read_stats2(None, C.byref(r), 47, None, None, 0, 2, None) == _lib.E_ARG
    assert lib.kmx_count_read_stats2(None, None, 47, None, None, 0, 2, None) == _lib.E_ARG


def test_rust_binding_carries_the_read_stats_calls():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert f"pub fn {name}(" in ffi
        assert f"pub fn {name[4:]}(ctx: &HipContext, " in lib_rs and f"{name}(ctx.0, " in lib_rs
    assert "pub const KMX_RS_SPAN" in ffi


def test_python_api_has_the_read_stats_methods():
    from kmers_amd.api import Context

    for name in NAMES:
        assert callable(getattr(Context, name[4:]))


def test_read_stats_span_decodes_a_row():
    import torch

    from kmers_amd import _lib
    from kmers_amd.api import read_stats_span

    rows = torch.zeros((3, 8), dtype=torch.int64)
    rows[0, _lib.RS_SPAN] = (20 << 32) | 7          # 20 windows from window 7
    rows[1, _lib.RS_SPAN] = 0                       # no solid window
    rows[2, _lib.RS_SPAN] = (1 << 32) | 0           # one window at the start
    first, end = read_stats_span(rows, 31)
    assert first.tolist() == [7, 0, 0] and end.tolist() == [7 + 20 + 30, 0, 31]
    first, end = read_stats_span(rows.reshape(-1), 5)      # the flat form count_read_stats takes as `out`
    assert first.tolist() == [7, 0, 0] and end.tolist() == [7 + 20 + 4, 0, 5]
