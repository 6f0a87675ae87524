"""kmx_bgzf_deflate without a GPU: the two calls are declared, bound, built and in the Rust FFI, with their flag; a null context is an
argument error; kmx_bgzf_deflate_bound is the size of zlib's level-0 image (every block stored) and 0 for a block size out of range;
write_fastx keeps the defaults it had."""
import ctypes as C
import inspect
import os
import re

import pytest

from tests import bgzf_np as B
from tests import bgzf_deflate_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_calls_declared_bound_built_and_in_rust():
    from kmers_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "kmx.hpp")).read()
    for name in ("kmx_bgzf_deflate", "kmx_bgzf_deflate_bound"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.SIGNATURES and re.search(r"pub fn %s\b" % name, ffi), name
    assert re.search(r"pub fn bgzf_deflate\b", rs) and re.search(r"inline std::string bgzf_deflate\(", hpp)
    consts = dict(re.findall(r"#define (KMX_BGZF_DEFLATE_\w+) (\d+)", hdr))
    assert consts == {"KMX_BGZF_DEFLATE_STORED": "1"} and _lib.BGZF_DEFLATE_STORED == 1 == K.STORED
    assert re.search(r"pub const KMX_BGZF_DEFLATE_STORED: \w+ = 1;", ffi)
    heads = [os.path.basename(h) for h in build._headers_of("kmx_bgzf.hip")]
    assert "kmx_bgzf_encode.h" in heads and "kmx_bgzf_decode.h" in heads
    assert not any(os.path.basename(h) == "kmx_bgzf_encode.h" for h in build._headers_of("kmx_fastx.hip"))
    lib = _lib.load()
    assert lib.kmx_bgzf_deflate and lib.kmx_bgzf_deflate_bound


def test_null_context_is_an_argument_error():
    from kmers_amd import _lib

    lib = _lib.load()
    info = (C.c_uint64 * 4)()
    assert lib.kmx_bgzf_deflate(None, None, 0, 0, 0, None, 0, None, info) == _lib.E_ARG


@pytest.mark.parametrize("bb", [1, 255, 256, 9000, 65279, 65280])
def test_bound_is_the_stored_image(bb):
    from kmers_amd import _lib

    lib = _lib.load()
    for n in (0, 1, bb - 1, bb, bb + 1, 3 * bb, 3 * bb + 7) if bb > 1 else (0, 1, 2, 300):
        text = bytes(i * 7 & 255 for i in range(n))
        want = len(B.write(text, 0, bb))
        assert lib.kmx_bgzf_deflate_bound(n, bb) == want == K.bound(n, bb), (n, bb)
    assert lib.kmx_bgzf_deflate_bound(200001, 0) == lib.kmx_bgzf_deflate_bound(200001, 65280)
    assert lib.kmx_bgzf_deflate_bound(10, 65281) == 0
    assert lib.kmx_bgzf_deflate_bound(2**40, 65280) == 2**40 + 36 * (2**40 // 65280) + 31 + 28      # (2^40 = 65280 q + 256)


def test_write_fastx_defaults_are_unchanged():
    from kmers_amd.api import Context

    p = inspect.signature(Context.write_fastx).parameters
    assert list(p) == ["self", "file", "bases", "n_reads", "read_len", "bgzf_level", "bgzf_device", "kw"]
    assert p["bgzf_level"].default is None and p["bgzf_device"].default is False and p["kw"].kind is inspect.Parameter.VAR_KEYWORD
    q = inspect.signature(Context.bgzf_deflate).parameters
    assert [(k, v.default) for k, v in q.items()][2:] == [("block_bytes", 65280), ("stored", False), ("offsets", False)]
