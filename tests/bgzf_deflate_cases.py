"""The texts kmx_bgzf_deflate and its host model (tests/cpp/bgzf_encode_check.cpp) are held to, seeded and small; the corpus file the
host program reads and the images it writes; and the zlib figures the size conditions compare with.  zlib is the reference."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import bgzf_np as B
from tests.fastx_cases import fastq_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "bgzf_encode_check.cpp")
STORED = 1      # KMX_BGZF_DEFLATE_STORED


def illumina_text(rng, n_reads=430, read_len=150, genome=20000):
    """(f): upper-case reads sampled from a random genome, quality strings in runs from few symbols, sequential names"""
    g = rng.choice(list(b"ACGT"), genome).astype(np.uint8)
    out = []
    for i in range(n_reads):
        at = int(rng.integers(0, genome - read_len))
        q = []
        while len(q) < read_len:
            q += [int(rng.choice(list(b"FFFF:,#")))] * int(rng.integers(1, 40))
        out += [b"@SIM:1:FCX:1:1101:%d:%d 1:N:0:ACGT" % (1000 + i, 2000 + 7 * i), g[at:at + read_len].tobytes(), b"+", bytes(q[:read_len])]
    return b"\n".join(out) + b"\n"


def no_repeat_text():
    """(j): over two symbols, no three bytes standing twice -- the de Bruijn word of order 3, written out: no match of any kind"""
    t = b"AAABABBBAA"
    assert len({t[i:i + 3] for i in range(len(t) - 2)}) == len(t) - 2
    return t


def enc_hash(four):
    """kmx_bgzf_encode.h's enc_hash: the table entry of four bytes (ENC_HASH_BITS = 11)"""
    return ((int.from_bytes(four, "little") * 2654435761) & 0xFFFFFFFF) >> 21


FAR_WORD = b"abcdefghijkl"      # (no 4 bytes of four-letter text, nor of its two seams with the word, share the entry of b"abcd")
FAR_AT = len(FAR_WORD) + 33000


def far_candidate_text():
    """(g), built: twelve bytes at the start and again 33012 bytes on, and between them four-letter text none of whose 4 bytes share
    the table entry of the word's first four -- so when the word comes again its entry still holds position 0, a candidate at a
    distance above 32768 that matches for 12 bytes and must be refused.  (Random bytes, as in g_far, overwrite every entry long
    before; and a token keeps distance - 1 in 15 bits, so a coder that took the candidate would write another distance.)"""
    rng = np.random.default_rng(35000)
    t = FAR_WORD + bytes(rng.choice(list(b"ACGT"), FAR_AT - len(FAR_WORD)).astype(np.uint8)) + FAR_WORD + bytes(rng.choice(list(b"ACGT"), 300).astype(np.uint8))
    h = enc_hash(FAR_WORD[:4])
    assert t[FAR_AT:FAR_AT + 12] == FAR_WORD and FAR_AT > 32768
    assert [p for p in range(FAR_AT + 1) if enc_hash(t[p:p + 4]) == h] == [0, FAR_AT]
    return t


# (h): the word twice, 124 bytes apart (the second in a later step of 64 positions than the first, so the table holds the first), and
# three bytes behind it; between them text that repeats at distance 10 only (distance symbol 6).  The second word's first half takes
# the table's candidate, the first word's second half at distance 117: distance symbol 13, which nothing else in the text takes; its
# second half (the next step) matches the first half 7 back and stops at the 'x'; the last positions hash nothing.
MATCH_THEN_3 = b"GATTACAGATTACA" + b"0123456789" * 11 + b"GATTACAGATTACA" + b"xyz"


def texts():
    """[(name, text)]: cases a..j of the list.  (b) is cut per block size by the callers: `cut_texts`."""
    rng = np.random.default_rng(20250131)
    r25 = rng.integers(0, 256, 25000, dtype=np.uint8).tobytes()
    out = [("a_empty", b""), ("a_1", b"A"), ("a_3", b"ACG"), ("a_4", b"ACGT"),
           ("c_one_byte", b"A" * 65280),
           ("d_random", rng.integers(0, 256, 200001, dtype=np.uint8).tobytes()),
           ("e_fastq", fastq_text(rng, 2000, fixed=150)),
           ("f_illumina", illumina_text(rng)),
           ("g_far", r25 + rng.integers(0, 256, 10000, dtype=np.uint8).tobytes() + r25),
           ("h_run_at_end", fastq_text(rng, 20, fixed=100) + b"#" * 1000),
           ("h_match_then_3", MATCH_THEN_3),
           ("g_far_candidate", far_candidate_text()),
           ("i_four_letters", bytes(rng.choice(list(b"ACGT"), 65280).astype(np.uint8))),
           ("j_no_match", no_repeat_text())]
    return out


def cut_texts(bb):
    """(b): exactly block_bytes, and one more"""
    rng = np.random.default_rng(77)
    t = fastq_text(rng, 450, fixed=150)
    assert len(t) > 65281
    return [(f"b_exact_{bb}", t[:bb]), (f"b_plus1_{bb}", t[:bb + 1])]


def entries(block_sizes):
    """[(name, block_bytes, flags, text)] over the corpus at the given block sizes"""
    out = []
    for bb in block_sizes:
        for name, t in texts() + cut_texts(bb):
            if bb == 256 and len(t) > 70000:
                t = t[:70000]              # (256-byte blocks: a few hundred blocks a text are enough)
            out.append((f"{name}@{bb}", bb, 0, t))
    return out


def compile_host(tmp_path):
    """-> (exe, sanitized)"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "bgzf_encode_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", SRC, "-o", exe]
    r = subprocess.run(base[:5] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[5:], capture_output=True, text=True)
    if r.returncode == 0:
        return exe, True
    r2 = subprocess.run(base, capture_output=True, text=True)
    assert r2.returncode == 0, r2.stderr[-3000:]
    return exe, False


def host_images(exe, ents, tmp_path, tag="corpus"):
    """the host model over `ents` -> [(image, stored blocks, DEFLATE blocks inside dynamic blocks)]"""
    corpus, images = tmp_path / (tag + ".bin"), tmp_path / (tag + ".img")
    corpus.write_bytes(struct.pack("<I", len(ents)) + b"".join(struct.pack("<III", bb, fl, len(t)) + t for _, bb, fl, t in ents))
    r = subprocess.run([exe, str(corpus), str(images)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert " 0 wrong" in r.stdout
    raw = images.read_bytes()
    assert struct.unpack_from("<I", raw)[0] == len(ents)
    out, at = [], 4
    for _ in ents:
        n, stored, deflate = struct.unpack_from("<III", raw, at)
        out.append((raw[at + 12:at + 12 + n], stored, deflate))
        at += 12 + n
    assert at == len(raw)
    return out


def bound(n_bytes, bb):
    """kmx_bgzf_deflate_bound: every piece stored as zlib's level 0 stores it -- 31 bytes around a piece below 32768 bytes, 36 from there on"""
    whole, rest = divmod(n_bytes, bb)
    return n_bytes + whole * (31 if bb < 32768 else 36) + ((31 if rest < 32768 else 36) if rest else 0) + 28


def huffman_only_size(text, bb=65280):
    """zlib's Z_HUFFMAN_ONLY stream over the same pieces, wrapped the same way"""
    return sum(len(B.block(text[i:i + bb], 6, zlib.Z_HUFFMAN_ONLY)) for i in range(0, len(text), bb)) + 28


def check_image(image, text, bb):
    """what holds for every image of `text`: gzip's bytes, the walk, every block's verdict with CRC, the bound; -> (block_offsets, text_offsets)"""
    import gzip

    assert gzip.decompress(image) == text
    bo, to, trailing, has_eof = B.walk(image)
    assert trailing == 0 and has_eof == 1
    assert len(bo) - 1 == (len(text) + bb - 1) // bb + 1
    for b in range(len(bo) - 1):
        s, e = int(bo[b]), int(bo[b + 1])
        assert e - s <= 65536
        ok, got = B.block_verdict(image, s, e, int(to[b + 1] - to[b]))
        assert ok and got == text[int(to[b]):int(to[b + 1])], b
    assert len(image) <= bound(len(text), bb)
    return bo, to


# The host model's size over zlib's on (e) and (f) at 65280 (profiles/bgzf_deflate_ratio.txt), rounded up to the next 0.05: what the
# size tests hold the model and the device to.
RATIO_BOUND_L1 = {"e_fastq": 1.05, "f_illumina": 0.85}     # measured: 1.0430 and 0.8223
