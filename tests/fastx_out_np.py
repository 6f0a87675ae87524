"""Host references of kmx_fastx_parse_names and kmx_fastx_format (include/kmx.h, "back to a file"), written straight from the
definitions there with bytes.split and b"".join: what tests/test_gpu_fastx_names.py and tests/test_gpu_fastx_format.py compare the
device's bytes and words with.  tests/test_fastx_out_np.py pins them: a formatted image parsed back is the batch it was made from.

A batch is (bases uint8[...], offsets[n + 1]) or, for uniform reads, (bases, None) with read_len; quals has the layout of bases;
names is a ragged batch of its own."""
import numpy as np

M64 = (1 << 64) - 1
FASTQ, FASTA = 1, 2


def fastq_names(text: bytes):
    """-> (names uint8[n_bytes], noffsets uint64[n + 1]): line i % 4 == 0 of the text as it stands ('@' included), every '\\r'
    dropped; what follows the last newline is a line only if it has a byte"""
    text = bytes(text)
    if not text:
        return np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    if text[:1] != b"@":
        raise ValueError("not a FASTQ text")
    lines = text.split(b"\n")
    if text.endswith(b"\n"):
        lines.pop()
    names = [ln.replace(b"\r", b"") for ln in lines[0::4]]
    off = np.zeros(len(names) + 1, np.uint64)
    off[1:] = np.cumsum([len(q) for q in names], dtype=np.uint64)
    return np.frombuffer(b"".join(names), dtype=np.uint8).copy(), off


def span(offsets, read_len, r):
    """(first byte, length) of read r under the rules of the read-preparation family: an offsets pair that descends counts as 0,
    2^31 bases or more count as 0"""
    if offsets is None:
        a, e = r * int(read_len), (r + 1) * int(read_len)
    else:
        a, e = int(offsets[r]), int(offsets[r + 1])
    n = e - a if e >= a else 0
    return a, (0 if n >= 1 << 31 else n)


def decimal_name(name_base, r):
    """name_base + r, wrapping mod 2^64, in decimal without leading zeros"""
    return b"%d" % ((int(name_base) + int(r)) & M64)


def records_np(bases, n_reads, read_len=0, offsets=None, quals=None, names=None, name_offsets=None, name_skip=1, name_base=0, fmt=FASTQ,
               line_width=0, qual_fill=ord("I")):
    """the records of the image, one bytes object each"""
    bases = bytes(np.asarray(bases, np.uint8).tobytes())
    quals = bytes(np.asarray(quals, np.uint8).tobytes()) if quals is not None else None
    names = bytes(np.asarray(names, np.uint8).tobytes()) if names is not None else None
    if fmt not in (FASTQ, FASTA) or (fmt == FASTQ and line_width != 0):
        raise ValueError("format")
    out = []
    for r in range(int(n_reads)):
        a, L = span(offsets, read_len, r)
        B = bases[a:a + L]
        if names is not None:
            na, nl = span(name_offsets, 0, r)
            skip = min(int(name_skip), nl)
            N = names[na + skip:na + nl]
        else:
            N = decimal_name(name_base, r)
        if fmt == FASTQ:
            Q = quals[a:a + L] if quals is not None else bytes([qual_fill]) * L
            out.append(b"@" + N + b"\n" + B + b"\n+\n" + Q + b"\n")
        else:
            W = int(line_width)
            lines = [B[i:i + W] for i in range(0, L, W)] if W and L else [B]
            out.append(b">" + N + b"\n" + b"".join(ln + b"\n" for ln in lines))
    return out


def format_np(*a, **kw):
    """-> (image uint8[n_bytes], rec_offsets uint64[n + 1])"""
    recs = records_np(*a, **kw)
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in recs], dtype=np.uint64)
    return np.frombuffer(b"".join(recs), dtype=np.uint8).copy(), off


def record_len(L, name_len, fmt, line_width=0):
    """the length of a record as kmx.h states it"""
    if fmt == FASTQ:
        return name_len + 2 * L + 6
    lines = max(1, -(-L // line_width)) if line_width else 1
    return name_len + 2 + L + lines
