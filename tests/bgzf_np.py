"""Host reference of the BGZF calls (kmx_bgzf_index, kmx_bgzf_inflate): a BGZF writer through zlib's raw DEFLATE, the walk of the block
chain, the soundness rule of kmx.h applied through zlib (block_verdict), and the list of cases the device and the host decoder are
held to.  zlib is the reference for the verdict and for every byte."""
import struct
import zlib

import numpy as np

from tests.fastx_cases import fastq_text

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEADER = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0"


def wrap(payload: bytes, text: bytes) -> bytes:
    """one BGZF block around a raw DEFLATE payload"""
    size = len(HEADER) + 2 + len(payload) + 8
    assert size <= 65536, size
    return HEADER + struct.pack("<H", size - 1) + payload + struct.pack("<II", zlib.crc32(text), len(text))


def block(text: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        payload = co.compress(text) + co.flush()
    else:
        payload = co.compress(text[:flush_at]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(text[flush_at:]) + co.flush()
    return wrap(payload, text)


def write(text: bytes, level=6, block_bytes=65280, eof=True) -> bytes:
    return b"".join(block(text[i:i + block_bytes], level) for i in range(0, len(text), block_bytes)) + (EOF_MARKER if eof else b"")


def header_at(f: bytes, p: int):
    """the size of the block whose header stands at p, or None"""
    h = f[p:p + 18]
    if len(h) < 18 or h[:4] != b"\x1f\x8b\x08\x04" or h[10:16] != b"\x06\0BC\x02\0":
        return None
    return struct.unpack("<H", h[16:18])[0] + 1


def walk(f: bytes):
    """the chain from byte 0 -> (block_offsets [n + 1], text_offsets [n + 1], trailing, has_eof); ValueError: no header at byte 0"""
    if header_at(f, 0) is None:
        raise ValueError("not BGZF")
    bo, to, p = [0], [0], 0
    last = None
    while True:
        size = header_at(f, p)
        if size is None or size < 28 or p + size > len(f):
            break
        to.append(to[-1] + struct.unpack("<I", f[p + size - 4:p + size])[0])
        last = f[p:p + size]
        p += size
        bo.append(p)
    return np.array(bo, np.uint64), np.array(to, np.uint64), len(f) - p, int(last == EOF_MARKER)


def block_verdict(f: bytes, start: int, end: int, isize_want=None, crc=True):
    """(sound, text): the rule of kmx.h for the block f[start:end) -- the header with BSIZE + 1 == end - start, a DEFLATE stream that zlib
    decodes to its end inside the payload, exactly ISIZE bytes (== isize_want, where given), the footer's CRC-32"""
    if end - start < 28 or end > len(f) or header_at(f, start) != end - start:
        return False, b""
    crc_want, isize = struct.unpack("<II", f[end - 8:end])
    if isize_want is not None and isize != isize_want:
        return False, b""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(f[start + 18:end - 8])
    except zlib.error:
        return False, b""
    if not d.eof or len(text) != isize:
        return False, b""
    if crc and zlib.crc32(text) != crc_want:
        return False, b""
    return True, text


def first_btype(blk: bytes) -> int:
    return (blk[18] >> 1) & 3


def _skewed(rng):
    """256 distinct bytes, frequencies falling by a factor of two every few symbols: code lengths well above 10"""
    out = []
    for s in range(256):
        out.append(bytes([s]) * max(1, 20000 >> (s // 6)))
    a = np.frombuffer(b"".join(out), np.uint8).copy()
    rng.shuffle(a)
    return a.tobytes()[:65000]


def single_block_cases():
    """[(name, block, text)]: cases 1..13 of the list, one BGZF block each"""
    rng = np.random.default_rng(20240607)
    fq = fastq_text(rng, 700, 50, 150)
    assert len(fq) > 66000
    cases = [("empty", EOF_MARKER, b""),
             ("one_byte_fixed", block(b"A", 9), b"A"),
             ("stored_largest", block(fq[:65280], 0), fq[:65280])]
    rnd = rng.integers(0, 256, 65280, dtype=np.uint8).tobytes()
    cases.append(("random_stored", block(rnd, 6), rnd))
    cases.append(("fixed_matches", block(fq[:20000], 6, zlib.Z_FIXED), fq[:20000]))
    for lv in (1, 6, 9):
        cases.append((f"dynamic_l{lv}", block(fq[:40000], lv), fq[:40000]))
    cases.append(("huffman_only", block(fq[:30000], 6, zlib.Z_HUFFMAN_ONLY), fq[:30000]))
    cases.append(("rle_max", block(b"A" * 65536, 6, zlib.Z_RLE), b"A" * 65536))
    cases.append(("period3", block(b"ACG" * 3000, 6), b"ACG" * 3000))
    p70 = bytes(rng.choice(list(b"ACGT"), 70).astype(np.uint8)) * 150
    cases.append(("period70", block(p70, 6), p70))
    cases.append(("full_flush", block(fq[:5000], 6, flush_at=1000), fq[:5000]))
    cases.append(("fastq_65536", block(fq[:65536], 6), fq[:65536]))
    sk = _skewed(rng)
    cases.append(("skewed_long_codes", block(sk, 9), sk))
    for n in (63, 64, 65):
        cases.append((f"ends_at_{n}", block(fq[:n], 6), fq[:n]))
    cases.append(("no_distance_code", no_distance_code_block(), b"AAAA"))
    return cases


def no_distance_code_block():
    """hand-made (zlib always writes two distance codes): a dynamic block whose distance set has no code at all -- HDIST = 1, its one
    length 0 -- and whose literal/length set is 'A' and end-of-block, one bit each; the text is b"AAAA" """
    out, n = 0, 0

    def put(v, k, msb=False):       # header fields least significant bit first, Huffman codes most significant bit first
        nonlocal out, n
        for i in range(k):
            out |= ((v >> (k - 1 - i if msb else i)) & 1) << n
            n += 1

    put(1, 1), put(2, 2), put(0, 5), put(0, 5), put(14, 4)              # BFINAL, dynamic, HLIT 257, HDIST 1, HCLEN 18
    cl = {18: 1, 0: 2, 1: 2}                                             # code-length code: 18 -> 0, 0 -> 10, 1 -> 11
    for sym in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1):
        put(cl.get(sym, 0), 3)
    zeros = lambda k: (put(0, 1, True), put(k - 11, 7))                  # symbol 18: 11..138 zeros
    one = lambda: put(3, 2, True)
    zeros(65), one(), zeros(138), zeros(52), one(), put(2, 2, True)      # 'A' = 1, 66..255 = 0, 256 = 1, the distance length 0
    for _ in range(4):
        put(0, 1, True)                                                  # 'A'
    put(1, 1, True)                                                      # end of block
    return wrap(out.to_bytes((n + 7) // 8, "little"), b"AAAA")


def nested_file():
    """a level-0 block whose payload is itself a complete BGZF block: a header stands verbatim inside stored data"""
    inner = block(b"@r\nACGT\n+\nIIII\n", 6) + EOF_MARKER
    return block(inner, 0) + block(b"tail", 6) + EOF_MARKER, inner + b"tail"


def files():
    """[(name, file bytes)]: every file of the case list"""
    cases = single_block_cases()
    out = [(name, blk) for name, blk, _ in cases]
    parts = []
    for i, (_, blk, _) in enumerate(cases):
        parts.append(blk)
        if i % 4 == 0:
            parts.append(EOF_MARKER)         # empty blocks in the middle
    cat = b"".join(parts)
    out.append(("concat_eof", cat + EOF_MARKER))
    out.append(("concat_no_eof", cat))
    out.append(("nested", nested_file()[0]))
    return out


def cut_files():
    whole = dict(files())["concat_eof"]
    return [(f"cut_{k}", whole[:len(whole) - k]) for k in range(1, 41)]


def host_text(f: bytes) -> bytes:
    bo, to, _, _ = walk(f)
    parts = []
    for b in range(len(bo) - 1):
        ok, text = block_verdict(f, int(bo[b]), int(bo[b + 1]), int(to[b + 1] - to[b]))
        assert ok, b
        parts.append(text)
    return b"".join(parts)


def flipped(f: bytes, bit: int) -> bytes:
    a = bytearray(f)
    a[bit >> 3] ^= 1 << (bit & 7)
    return bytes(a)


def corpus_bytes(entries) -> bytes:
    """the corpus file of tests/cpp/bgzf_host_check.cpp: per entry (block, sound, room, text) u32 block length, u32 expected verdict
    (1 sound), u32 room (the bytes the index gives the block), u32 text length, the block, the text (the bytes of a sound block)"""
    out = [struct.pack("<I", len(entries))]
    for blk, sound, room, text in entries:
        out.append(struct.pack("<IIII", len(blk), int(sound), room, len(text)) + blk + text)
    return b"".join(out)


def three_block_file():
    """the file of the corruption test: three dynamic blocks; -> (file, block_offsets, text_offsets, texts)"""
    rng = np.random.default_rng(99)
    texts = [fastq_text(rng, 12, 40, 90), fastq_text(rng, 25, 40, 120), fastq_text(rng, 9, 40, 90)]
    f = b"".join(block(t, 6) for t in texts)
    bo, to, trailing, _ = walk(f)
    assert len(bo) == 4 and trailing == 0
    return f, bo, to, texts


# The seed of the corruption test's 200 flips: by the host reference alone (block_verdict), three of them fall in the six ignored
# header bytes and stay sound, 197 do not -- both verdicts occur (of seeds 1..39, twenty have no sound flip at all).
FLIP_SEED = 13


def flip_bits(n_bits: int, count: int, seed: int):
    return [int(x) for x in np.random.default_rng(seed).integers(0, n_bits, count)]


def dynamic_code_lengths(blk: bytes):
    """the literal/length and distance code lengths of the first DEFLATE block of a BGZF block (it must be dynamic), read bit by bit"""
    data, pos = blk[18:-8], 0

    def bits(k):
        nonlocal pos
        v = 0
        for i in range(k):
            v |= ((data[pos >> 3] >> (pos & 7)) & 1) << i
            pos += 1
        return v

    assert bits(3) >> 1 == 2
    hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[i]] = bits(3)
    codes, code = {}, 0
    for ln in range(1, 8):
        for s in range(19):
            if cl[s] == ln:
                codes[(ln, code)] = s
                code += 1
        code <<= 1
    lens = []
    while len(lens) < hlit + hdist:
        c, ln = 0, 0
        while (ln, c) not in codes:
            c, ln = (c << 1) | bits(1), ln + 1
            assert ln <= 7
        s = codes[(ln, c)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + bits(2))
        else:
            lens += [0] * (3 + bits(3) if s == 17 else 11 + bits(7))
    return lens[:hlit], lens[hlit:hlit + hdist]
