"""kmx_count_setop(2) / kmx_count_compare(2) without a GPU: the symbols are exported, bound and declared, argument errors come back
as codes (never a crash), the Rust binding carries the calls, Context has the methods, and the ratios derived from a comparison
record are right on hand-made records."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("kmx_count_setop", "kmx_count_setop2", "kmx_count_compare", "kmx_count_compare2")
CONSTANTS = {"KMX_SETOP_INTERSECT": 0, "KMX_SETOP_UNION": 1, "KMX_SETOP_SUBTRACT": 2, "KMX_SETOP_SYMDIFF": 3, "KMX_SETOP_COUNTER_SUBTRACT": 4,
             "KMX_RULE_SUM": 0, "KMX_RULE_MIN": 1, "KMX_RULE_MAX": 2, "KMX_RULE_LEFT": 3, "KMX_RULE_RIGHT": 4}


def test_setop_symbols_are_exported_bound_and_declared():
    from kmers_amd import _lib

    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert f"int {name}(kmx_ctx *ctx," in hdr
    for name, value in CONSTANTS.items():
        assert f"#define {name} {value}\n" in hdr
        assert getattr(_lib, name[4:]) == value
    assert "} kmx_table_compare;" in hdr
    assert C.sizeof(_lib.TableCompare) == 72
    assert [f for f, _ in _lib.TableCompare._fields_] == ["n_both", "n_only_a", "n_only_b", "sum_a", "sum_b", "sum_a_both", "sum_b_both",
                                                          "sum_min", "sum_max"]
    assert "#define KMX_VERSION 2" in hdr and lib.kmx_version() == 2
    # the tile the boundary tests are built around is the kernel file's
    src = open(os.path.join(ROOT, "kmers_amd", "csrc", "kmx_count_setop.hip")).read()
    assert "SETOP_TILE = CT * SETOP_IPT" in src and "SETOP_IPT = 8;" in src and _lib.SETOP_TILE == 256 * 8


def test_setop_argument_errors_are_codes_not_crashes():
    from kmers_amd import _lib

    lib = _lib.load()
    n = C.c_uint64(7)
    rec = _lib.TableCompare()
    fake = C.c_void_p(0x1000)   # stands for a context: every check below fails before the context is touched
    for f in (lib.kmx_count_setop, lib.kmx_count_setop2):
        assert f(None, 0, 0, None, None, 0, None, None, 0, None, None, 0, C.byref(n)) == _lib.E_ARG      # NULL context
        assert f(fake, 0, 0, None, None, 0, None, None, 0, None, None, 0, None) == _lib.E_ARG             # NULL h_n_out
        assert f(fake, 5, 0, None, None, 0, None, None, 0, None, None, 0, C.byref(n)) == _lib.E_ARG      # unknown op
        assert f(fake, 0xFFFFFFFF, 0, None, None, 0, None, None, 0, None, None, 0, C.byref(n)) == _lib.E_ARG
        assert f(fake, 0, 5, None, None, 0, None, None, 0, None, None, 0, C.byref(n)) == _lib.E_ARG      # unknown rule
        assert f(fake, 1, 0xFFFFFFFF, None, None, 0, None, None, 0, None, None, 0, C.byref(n)) == _lib.E_ARG
        for op in (_lib.SETOP_SUBTRACT, _lib.SETOP_SYMDIFF, _lib.SETOP_COUNTER_SUBTRACT):                 # a rule where none is taken
            for rule in (_lib.RULE_MIN, _lib.RULE_MAX, _lib.RULE_LEFT, _lib.RULE_RIGHT):
                assert f(fake, op, rule, None, None, 0, None, None, 0, None, None, 0, C.byref(n)) == _lib.E_ARG
        assert f(fake, 0, 0, None, None, 0, None, None, 0, fake, None, 0, C.byref(n)) == _lib.E_ARG      # one output NULL
    for f in (lib.kmx_count_compare, lib.kmx_count_compare2):
        assert f(None, None, None, 0, None, None, 0, C.byref(rec)) == _lib.E_ARG
        assert f(fake, None, None, 0, None, None, 0, None) == _lib.E_ARG
    assert n.value == 7   # nothing was written on the way out


def test_rust_binding_carries_the_setop_calls():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert f"pub fn {name}(" in ffi
        assert f"pub fn {name[4:]}(ctx: &HipContext, " in lib_rs and f"{name}(ctx.0, " in lib_rs
    for name, value in CONSTANTS.items():
        assert f"pub const {name}: u32 = {value};" in ffi
    assert "pub struct kmx_table_compare {" in ffi


def test_python_api_has_the_setop_methods():
    from kmers_amd.api import Context

    for name in NAMES:
        assert callable(getattr(Context, name[4:]))
    for base in ("count_intersect", "count_union", "count_subtract", "count_symdiff", "count_counter_subtract"):
        assert callable(getattr(Context, base)) and callable(getattr(Context, base + "2"))


def test_derived_ratios_of_hand_made_records():
    from kmers_amd.api import TableComparison

    # disjoint: a = {x: 2, y: 3}, b = {z: 4}
    d = TableComparison(n_both=0, n_only_a=2, n_only_b=1, sum_a=5, sum_b=4, sum_a_both=0, sum_b_both=0, sum_min=0, sum_max=9)
    assert (d.jaccard, d.containment_a, d.containment_b, d.weighted_jaccard, d.bray_curtis) == (0.0, 0.0, 0.0, 0.0, 1.0)
    # identical: a = b = {x: 2, y: 3, z: 5}
    s = TableComparison(n_both=3, n_only_a=0, n_only_b=0, sum_a=10, sum_b=10, sum_a_both=10, sum_b_both=10, sum_min=10, sum_max=10)
    assert (s.jaccard, s.containment_a, s.containment_b, s.weighted_jaccard, s.bray_curtis) == (1.0, 1.0, 1.0, 1.0, 0.0)
    # one empty: a = {}, b = {x: 1, y: 1}
    e = TableComparison(n_both=0, n_only_a=0, n_only_b=2, sum_a=0, sum_b=2, sum_a_both=0, sum_b_both=0, sum_min=0, sum_max=2)
    assert (e.jaccard, e.containment_a, e.containment_b, e.weighted_jaccard, e.bray_curtis) == (0.0, 0.0, 0.0, 0.0, 1.0)
    # both empty: every denominator is 0
    z = TableComparison(0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert (z.jaccard, z.containment_a, z.containment_b, z.weighted_jaccard, z.bray_curtis) == (0.0, 0.0, 0.0, 0.0, 0.0)
    # a mixed one: a = {x: 2, y: 6}, b = {y: 2, z: 2}
    m = TableComparison(n_both=1, n_only_a=1, n_only_b=1, sum_a=8, sum_b=4, sum_a_both=6, sum_b_both=2, sum_min=2, sum_max=10)
    assert m.jaccard == 1 / 3 and m.containment_a == 0.5 and m.containment_b == 0.5 and m.weighted_jaccard == 0.2
    assert abs(m.bray_curtis - (1 - 4 / 12)) < 1e-15
