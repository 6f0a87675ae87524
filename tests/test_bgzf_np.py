"""Pins the host reference of the BGZF calls (tests/bgzf_np.py) and their binding (CPU only): every file of the case list round-trips
through Python's gzip; the EOF marker is the 28 standard bytes; the list holds what it says it holds (all three block types, codes
longer than the primary table's ten bits, a distance set with no code, a header pattern inside stored data); the host walk finds the
blocks; bgzf_compress keeps every block within 64 KiB; the two calls are declared, bound, listed for the build and in the Rust FFI."""
import ctypes as C
import gzip
import os
import re
import zlib

import numpy as np
import pytest

from tests import bgzf_np as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = B.single_block_cases()
FILES = B.files()


@pytest.mark.parametrize("name", [n for n, _ in FILES])
def test_files_round_trip_through_gzip(name):
    f = dict(FILES)[name]
    assert gzip.decompress(f) == B.host_text(f)


def test_single_cases_hold_their_text():
    for name, blk, text in CASES:
        ok, got = B.block_verdict(blk, 0, len(blk), len(text))
        assert ok and got == text, name
        assert len(blk) <= 65536


def test_eof_marker_is_the_standard_one():
    assert len(B.EOF_MARKER) == 28 and B.EOF_MARKER == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    assert B.block(b"", 6) == B.EOF_MARKER
    assert gzip.decompress(B.EOF_MARKER) == b""


def test_case_list_holds_what_it_says():
    c = {name: blk for name, blk, _ in CASES}
    assert {B.first_btype(blk) for blk in c.values()} == {0, 1, 2}
    assert B.first_btype(c["one_byte_fixed"]) == 1 and B.first_btype(c["fixed_matches"]) == 1
    assert B.first_btype(c["stored_largest"]) == 0 and B.first_btype(c["random_stored"]) == 0
    assert 65280 + 5 + 26 <= len(c["stored_largest"]) <= 65536
    for lv in (1, 6, 9):
        assert B.first_btype(c[f"dynamic_l{lv}"]) == 2
    lit, dist = B.dynamic_code_lengths(c["skewed_long_codes"])
    assert max(lit) > 10                                    # the decode path behind the primary table
    lit, dist = B.dynamic_code_lengths(c["huffman_only"])
    assert max(dist) <= 1 and lit[256] > 0                  # literals only (zlib still writes its two one-bit distance codes)
    lit, dist = B.dynamic_code_lengths(c["no_distance_code"])
    assert dist == [0] and [i for i, v in enumerate(lit) if v] == [65, 256]     # a distance set with no code at all
    assert len(dict((n, t) for n, _, t in CASES)["rle_max"]) == 65536
    f, text = B.nested_file()
    assert f.count(B.HEADER[:4]) > len(B.walk(f)[0]) - 1    # a header pattern that is no block
    assert B.host_text(f) == text


def test_walk_finds_the_blocks():
    f = dict(FILES)["concat_eof"]
    bo, to, trailing, has_eof = B.walk(f)
    assert trailing == 0 and has_eof == 1 and int(bo[-1]) == len(f) and int(to[-1]) == len(gzip.decompress(f))
    assert len(bo) - 1 == len(CASES) + sum(1 for i in range(len(CASES)) if i % 4 == 0) + 1
    assert B.walk(dict(FILES)["concat_no_eof"])[2:] == (0, 0)
    bo2, _, trailing2, eof2 = B.walk(dict(FILES)["nested"])
    assert len(bo2) - 1 == 3 and trailing2 == 0 and eof2 == 1
    for name, cut in B.cut_files():
        cb, ct, ctr, ceof = B.walk(cut)
        k = len(f) - len(cut)
        assert ceof == 0 and len(cb) < len(bo) and int(cb[-1]) + ctr == len(cut), name
        assert np.array_equal(cb, bo[:len(cb)]) and np.array_equal(ct, to[:len(ct)])
        assert ctr == (28 - k if k <= 28 else len(cut) - int(bo[-3]))     # (cut by 28: the marker is gone whole, the file is sound)
    with pytest.raises(ValueError):
        B.walk(gzip.compress(b"plain gzip"))
    with pytest.raises(ValueError):
        B.walk(b"@r\nACGT\n+\nIIII\n")


def test_verdict_rejects_what_the_rule_rejects():
    blk, text = CASES[5][1], CASES[5][2]
    assert B.block_verdict(blk, 0, len(blk), len(text))[0]
    assert not B.block_verdict(blk, 0, len(blk), len(text) + 1)[0]
    crc_bit = 8 * (len(blk) - 8)
    assert not B.block_verdict(B.flipped(blk, crc_bit), 0, len(blk))[0] and B.block_verdict(B.flipped(blk, crc_bit), 0, len(blk), crc=False)[0]
    assert B.block_verdict(B.flipped(blk, 8 * 5), 0, len(blk))[0]            # the six ignored header bytes
    assert not B.block_verdict(B.flipped(blk, 8 * 12), 0, len(blk))[0]
    assert not B.block_verdict(blk + b"x", 0, len(blk) + 1)[0]


def test_bgzf_compress_blocks_and_round_trip():
    from kmers_amd.api import BGZF_EOF, bgzf_compress

    assert BGZF_EOF == B.EOF_MARKER
    rng = np.random.default_rng(4)
    data = rng.integers(0, 256, 200001, dtype=np.uint8).tobytes()          # incompressible: the largest blocks there are
    for level in (0, 1, 6, 9):
        f = bgzf_compress(data, level)
        bo, to, trailing, has_eof = B.walk(f)
        assert trailing == 0 and has_eof == 1 and int(np.diff(bo.astype(np.int64)).max()) <= 65536
        assert gzip.decompress(f) == data and B.host_text(f) == data
    assert bgzf_compress(b"") == B.EOF_MARKER
    assert bgzf_compress(b"abc", 6, 2) == B.block(b"ab", 6) + B.block(b"c", 6) + B.EOF_MARKER
    with pytest.raises(ValueError):
        bgzf_compress(b"abc", 6, 65281)


def test_calls_declared_bound_built_and_in_rust():
    from kmers_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "kmx.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name in ("kmx_bgzf_index", "kmx_bgzf_inflate"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.SIGNATURES and re.search(r"pub fn %s\b" % name, ffi), name
    assert "kmx_bgzf.hip" in build.SOURCES
    assert any(os.path.basename(h) == "kmx_bgzf_decode.h" for h in build._headers_of("kmx_bgzf.hip"))
    assert not any(os.path.basename(h) == "kmx_bgzf_decode.h" for h in build._headers_of("kmx_fastx.hip"))
    consts = dict(re.findall(r"#define (KMX_BGZF_\w+) (\d+)", hdr))
    assert int(consts["KMX_BGZF_NO_CRC"]) == _lib.BGZF_NO_CRC == 1
    for k, v in consts.items():
        if k.startswith("KMX_BGZF_ST_"):
            assert getattr(_lib, k[4:]) == int(v) and int(v) in _lib.BGZF_ST_NAMES and re.search(r"pub const %s: \w+ = %s;" % (k, v), ffi), k
    assert len([k for k in consts if k.startswith("KMX_BGZF_ST_")]) == 14


def test_null_context_is_an_argument_error():
    from kmers_amd import _lib

    lib = _lib.load()
    info = (C.c_uint64 * 4)()
    assert lib.kmx_bgzf_index(None, None, 0, None, None, 0, info) == _lib.E_ARG
    assert lib.kmx_bgzf_inflate(None, None, 0, None, None, 0, 0, None, 0, None, None) == _lib.E_ARG
