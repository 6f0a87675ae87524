"""kmx_reads_complexity at the boundary, without a GPU: include/kmx.h declares it with eleven arguments and the eight KMX_RX_* words,
kmers_amd/_lib.py binds the same signature and carries the same constants, the host reference (tests/complexity_np.py) numbers the
words the same way, and the library exports the symbol and refuses its argument errors before it touches a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"kmx_ctx *": C.c_void_p, "uint8_t *": C.c_void_p, "uint64_t *": C.c_void_p, "uint32_t": C.c_uint32}


def _header():
    return open(os.path.join(ROOT, "include", "kmx.h")).read()


def test_rx_constants_agree_with_the_header():
    from kmers_amd import _lib
    from tests import complexity_np as X

    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define KMX_RX_([A-Z]+)\s+(\d+)u", _header())}
    assert defs == {"WORDS": 8, "KEEP": 0, "BASES": 1, "TAIL": 2, "HEAD": 3, "AC": 4, "GT": 5, "DIFF": 6, "DUST": 7}
    for name, v in defs.items():
        assert getattr(_lib, "RX_" + name) == v and getattr(X, "RX_" + name) == v, name


def test_signature_agrees_with_the_header():
    from kmers_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+kmx_reads_complexity\s*\(([^)]*)\)", src)
    assert m, "kmx_reads_complexity is not declared in include/kmx.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert [p.rsplit(" ", 1)[1].lstrip("*") for p in params] == ["ctx", "reads", "tail_bases", "head_bases", "min_len", "err_num", "err_den", "penalty",
                                                                 "dust_max", "d_masked", "d_rows"]
    restype, argtypes = _lib.SIGNATURES["kmx_reads_complexity"]
    assert restype is C.c_int and len(argtypes) == len(params)
    for p, t in zip(params, argtypes):
        if p.startswith("const kmx_reads *"):
            assert t is C.POINTER(_lib.Reads), p
        else:
            want = next(v for k, v in C_TYPES.items() if p.replace("const ", "").startswith(k))
            assert t is want, p


def test_argument_errors_need_no_device():
    from kmers_amd import _lib

    lib = _lib.load()
    reads = _lib.Reads(None, 0, 16, None)
    assert lib.kmx_reads_complexity(None, C.byref(reads), 4, 0, 10, 1, 10, 2, 122, None, None) == _lib.E_ARG
