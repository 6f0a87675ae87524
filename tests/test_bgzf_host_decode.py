"""The serial core of the device's BGZF decoder (kmers_amd/csrc/kmx_bgzf_decode.h) on the host, under a sanitizer: tests/cpp/
bgzf_host_check.cpp is compiled with -fsanitize=address,undefined (without, where the compiler has no sanitizer runtime) and run as a
child process over a corpus this test writes -- every block of every file of tests/bgzf_np.py, and single-bit flips of them, the
header and footer included -- with zlib's verdict and bytes beside each.  A clean exit says: the verdicts and the bytes are zlib's, and
no index went out of bounds on the way.  CPU only; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

from tests import bgzf_np as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "bgzf_host_check.cpp")


def _entries():
    out = []
    for name, f in B.files():
        bo, to, _, _ = B.walk(f)
        for b in range(len(bo) - 1):
            s, e, room = int(bo[b]), int(bo[b + 1]), int(to[b + 1] - to[b])
            ok, text = B.block_verdict(f, s, e, room)
            assert ok, (name, b)
            out.append((f[s:e], True, room, text))
    # flips anywhere in a block, judged by zlib: the blocks of the corruption test's file, and some of every single case
    f3, bo3, to3, _ = B.three_block_file()
    s, e, room = int(bo3[1]), int(bo3[2]), int(to3[2] - to3[1])
    for bit in B.flip_bits(8 * (e - s), 200, B.FLIP_SEED) + [8 * 18 + k for k in range(300)]:
        blk = B.flipped(f3[s:e], bit)
        ok, text = B.block_verdict(blk, 0, len(blk), room)
        out.append((blk, ok, room, text))
    for i, (name, blk, text) in enumerate(B.single_block_cases()):
        for bit in B.flip_bits(8 * len(blk), 30, 100 + i) + [8 * 18 + k for k in range(40)]:
            bad = B.flipped(blk, bit)
            ok, t = B.block_verdict(bad, 0, len(bad), len(text))
            out.append((bad, ok, len(text), t))
    return out


def _compile(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "bgzf_host_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", SRC, "-o", exe]
    r = subprocess.run(base[:5] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[5:], capture_output=True, text=True)
    if r.returncode == 0:
        return exe, True
    r2 = subprocess.run(base, capture_output=True, text=True)
    assert r2.returncode == 0, r2.stderr[-3000:]
    return exe, False


def test_host_decoder_matches_zlib_under_sanitizer(tmp_path):
    entries = _entries()
    assert sum(1 for e in entries if e[1]) > 40 and sum(1 for e in entries if not e[1]) > 400
    corpus = tmp_path / "corpus.bin"
    corpus.write_bytes(B.corpus_bytes(entries))
    exe, sanitized = _compile(tmp_path)
    r = subprocess.run([exe, str(corpus)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "0 wrong" in r.stdout
    if not sanitized:
        pytest.skip("the compiler has no sanitizer runtime here: the check ran and passed without -fsanitize=address,undefined")
