"""kmx_fastx_format on the GPU: a batch laid out as a FASTQ / FASTA image (kmx_fastx_format.hip), and what the Python layer builds on
it (Context.fastx_format, write_fastx, fastq_records, Unitigs.write_fasta).

Every comparison is equality of every byte of the image and every record offset with the host reference tests/fastx_out_np.py
(pinned in tests/test_fastx_out_np.py): there is no tolerance anywhere.  The raw calls go through `run_format`, which makes a
count-only call, then hands the ABI buffers that are longer than the result and filled with a sentinel, and looks at every byte in
front of a shifted d_text and behind n_bytes and at every word behind the n_reads + 1 record offsets.

The copy's grid is NOT capped: a block per 64 KiB of the image, however many that are (an image is below 2^44 bytes), and the
plan's kernels a block per 2048 records; there is no second sweep to test.  The cases below with more than one block: 3000 six-byte
records (one block, more records than the 512 staged in LDS), the 64 KiB segments (five blocks), the round trips (several)."""
import ctypes as C
import io

import numpy as np
import pytest

from tests import fastx_out_np as F
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import random_reads, u64
from tests.fastx_cases import fastq_text
from tests.reads_dev import SENT, SENT_WORD, dev_bytes, dev_words, ptr, ragged

pytestmark = pytest.mark.gpu

OK, E_ARG, E_NOMEM = 0, 1, 6
AUTO, FASTQ, FASTA, SAME_TEXT = 0, 1, 2, 0x100
GUARD = 64           # sentinel bytes behind d_text
SENT_U64 = np.uint64(SENT_WORD & (2**64 - 1))


class Src:
    """the sources of a call on the host and on the device: reads (offsets None = uniform reads of read_len bases), quality bytes
    laid out as the bases are, a batch of names; each at a byte phase of its own"""

    def __init__(self, ctx, bases, n, read_len=0, offsets=None, quals=None, names=None, name_offsets=None, shifts=(0, 0, 0)):
        from kmers_amd._lib import Reads

        self.ctx, self.n, self.read_len = ctx, int(n), int(read_len)
        self.h = dict(bases=np.asarray(bases, np.uint8), offsets=offsets, quals=quals, names=names, name_offsets=name_offsets)
        self.d_bases = dev_bytes(ctx, self.h["bases"], shifts[0])
        self.d_off = dev_words(ctx, offsets)
        self.d_quals = dev_bytes(ctx, np.asarray(quals, np.uint8), shifts[1]) if quals is not None else None
        self.d_names = dev_bytes(ctx, np.asarray(names, np.uint8), shifts[2]) if names is not None else None
        self.d_noff = dev_words(ctx, name_offsets)
        self.reads = Reads(self.d_bases.data_ptr() if self.n else None, self.n, self.read_len, self.d_off.data_ptr() if offsets is not None else None)
        self.names = Reads(self.d_names.data_ptr(), self.n, 0, self.d_noff.data_ptr()) if names is not None else None

    def want(self, **kw):
        h = self.h
        return F.format_np(h["bases"], self.n, self.read_len, h["offsets"], quals=h["quals"] if kw.get("use_quals", True) else None, names=h["names"],
                           name_offsets=h["name_offsets"], **{k: v for k, v in kw.items() if k != "use_quals"})


def run_format(s, fmt=FASTQ, name_skip=1, name_base=0, line_width=0, qual_fill=ord("I"), out_shift=0, use_quals=True, want_offsets=True):
    """kmx_fastx_format through the raw ABI: a count-only call, then the write into guarded buffers; everything is compared with the
    reference -> the image on the host"""
    import torch

    ctx = s.ctx
    want_t, want_o = s.want(fmt=fmt, name_skip=name_skip, name_base=name_base, line_width=line_width, qual_fill=qual_fill, use_quals=use_quals)
    head = (ctx._h, C.byref(s.reads), ptr(s.d_quals) if use_quals else None, C.byref(s.names) if s.names is not None else None, name_skip,
            name_base & (2**64 - 1), fmt, line_width, qual_fill)
    nb = C.c_uint64(99)
    st = ctx.lib.kmx_fastx_format(*head, None, None, 0, C.byref(nb))
    assert st == OK and nb.value == len(want_t), (st, nb.value, len(want_t))
    n_bytes = nb.value
    raw = torch.full((n_bytes + GUARD + 32,), SENT, dtype=torch.uint8, device=ctx.device)
    out = raw[out_shift:out_shift + n_bytes + GUARD]
    off = torch.full((s.n + 2,), SENT_WORD, dtype=torch.int64, device=ctx.device)
    nb = C.c_uint64(99)
    st = ctx.lib.kmx_fastx_format(*head, ptr(out), ptr(off) if want_offsets else None, n_bytes, C.byref(nb))
    assert st == OK and nb.value == n_bytes
    h_raw, h_off = raw.cpu().numpy(), u64(off)
    h_out = h_raw[out_shift:out_shift + n_bytes]
    if not np.array_equal(h_out, want_t):
        at = int(np.nonzero(h_out != want_t)[0][0])
        raise AssertionError(f"bytes differ from byte {at} of {n_bytes} on: {h_out[at:at + 24].tobytes()!r} for {want_t[at:at + 24].tobytes()!r}")
    assert (h_raw[:out_shift] == SENT).all() and (h_raw[out_shift + n_bytes:] == SENT).all(), "a byte outside the image was written"
    if s.n and want_offsets:
        assert np.array_equal(h_off[:s.n + 1], want_o), "record offsets"
        assert h_off[s.n + 1] == SENT_U64, "the word after the record offsets was written"
    else:
        assert (h_off == SENT_U64).all()          # n_reads == 0 is a no-op: not even offsets[0]
    if s.n and want_offsets:
        # count only with d_rec_offsets: the offsets are still written
        off2 = torch.full((s.n + 2,), SENT_WORD, dtype=torch.int64, device=ctx.device)
        assert ctx.lib.kmx_fastx_format(*head, None, ptr(off2), 0, C.byref(nb)) == OK and nb.value == n_bytes
        assert np.array_equal(u64(off2)[:s.n + 1], want_o) and u64(off2)[s.n + 1] == SENT_U64
    return h_out


def _src(ctx, rng, read_lens, name_lens, first=(0, 0), shifts=(0, 0, 0)):
    reads = [bytes(random_reads(rng, int(n))) for n in read_lens]
    quals = [bytes(rng.integers(33, 74, int(n)).astype(np.uint8)) for n in read_lens]
    names = [bytes(rng.integers(97, 123, int(n)).astype(np.uint8)) for n in name_lens]
    bases, off = ragged(reads, first[0])
    q, _ = ragged(quals, first[0])
    nm, noff = ragged(names, first[1])
    return Src(ctx, bases, len(reads), 0, off, q, nm, noff, shifts)


# ---------------------------------------------------------------- the smallest shapes
def test_no_reads_and_one_read(ctx):
    rng = np.random.default_rng(1)
    empty = Src(ctx, np.zeros(0, np.uint8), 0, 0, np.zeros(1, np.uint64), np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert len(run_format(empty)) == 0 and len(run_format(empty, fmt=FASTA, line_width=3)) == 0
    one = _src(ctx, rng, [23], [9])
    assert run_format(one, name_skip=0).tobytes().count(b"\n") == 4
    assert run_format(one, fmt=FASTA, line_width=10).tobytes().count(b"\n") == 4
    # one record with an empty read and an empty name: six bytes of FASTQ, three of FASTA
    nothing = _src(ctx, rng, [0], [0])
    assert run_format(nothing, name_skip=0, out_shift=5).tobytes() == b"@\n\n+\n\n"
    assert run_format(nothing, name_skip=0, fmt=FASTA, out_shift=14).tobytes() == b">\n\n"


def test_six_byte_records(ctx):
    """3000 records of six bytes: every 16-byte piece holds several records, and more records begin inside the block's 64 KiB than
    the 512 that are staged in LDS, so most pieces find their first record by bisection in the global offsets"""
    rng = np.random.default_rng(2)
    s = _src(ctx, rng, [0] * 3000, [0] * 3000)
    for shift in (0, 7):
        assert run_format(s, name_skip=0, out_shift=shift).tobytes() == b"@\n\n+\n\n" * 3000
    assert run_format(s, name_skip=0, fmt=FASTA, out_shift=3).tobytes() == b">\n\n" * 3000


@pytest.mark.parametrize("phase", range(4))
def test_short_records_every_alignment(ctx, phase):
    """lengths 0..40 of reads and names; every output alignment 0..15; the byte phases of bases, quality bytes and names vary
    independently over the four cases (phase, phase + 1, 2 phase + 3 mod 4 with d_offsets[0] adding to them)"""
    rng = np.random.default_rng(10 + phase)
    n = 600
    rl, nl = rng.integers(0, 41, n), rng.integers(0, 41, n)
    rl[100:140] = 0
    nl[120:170] = 0
    shifts = (phase, (phase + 1) & 3, (2 * phase + 3) & 3)
    s = _src(ctx, rng, rl, nl, first=(phase, 3 - phase), shifts=shifts)
    assert {int(x) for x in rl} == set(range(41)) == {int(x) for x in nl}
    for A in range(16):
        run_format(s, out_shift=A, want_offsets=A % 4 == 0)
        run_format(s, fmt=FASTA, line_width=(0, 1, 7, 16)[A & 3], out_shift=A, want_offsets=False)


@pytest.mark.parametrize("pb,pq,pn", [(b, q, n) for b in range(4) for q in range(4) for n in range(4) if (b + 2 * q + 3 * n) % 4 == 0])
def test_source_phases_crossed(ctx, pb, pq, pn):
    """the byte phases of the three sources crossed (sixteen of the 64 triples, every pair of phases of two sources among them)"""
    rng = np.random.default_rng(100 + 16 * pb + 4 * pq + pn)
    s = _src(ctx, rng, rng.integers(0, 41, 200), rng.integers(0, 41, 200), shifts=(pb, pq, pn))
    run_format(s, out_shift=(5 * pb + pq + 3 * pn) & 15)


def test_long_segments(ctx):
    """one record whose name, bases and quality bytes are each longer than 64 KiB: blocks begin inside every kind of segment"""
    rng = np.random.default_rng(3)
    s = _src(ctx, rng, [70001], [66000], first=(3, 1), shifts=(1, 2, 3))
    text = run_format(s, out_shift=9)
    # the blocks' first bytes: byte 65536 b - 9 of the image
    kinds = set()
    for b in range(1, (len(text) + 9) // 65536 + 1):
        p = 65536 * b - 9
        kinds.add("name" if p < 66001 else "bases" if p < 66001 + 70002 else "quals")
    assert kinds == {"name", "bases", "quals"}
    run_format(s, fmt=FASTA, line_width=60, out_shift=2)
    run_format(s, fmt=FASTA, line_width=0, out_shift=15)


def test_layouts_of_the_reads(ctx):
    rng = np.random.default_rng(4)
    # uniform reads (d_offsets == NULL) with ragged names, and name_skip 0, 1 and past the end of every name
    n, L = 700, 33
    bases, quals = random_reads(rng, n * L + 3), rng.integers(33, 74, n * L + 3).astype(np.uint8)
    nm, noff = ragged([b"@n%d" % i for i in range(n)], first=2)
    s = Src(ctx, bases, n, L, None, quals, nm, noff, shifts=(3, 1, 2))
    for skip in (0, 1, 2, 5, 2**32 - 1):
        run_format(s, name_skip=skip, out_shift=skip & 15)
    run_format(s, fmt=FASTA, line_width=11, name_skip=1)
    # ragged reads with d_offsets[0] > 0 and a descending offsets pair (an empty read)
    s = _src(ctx, rng, rng.integers(0, 60, 50), rng.integers(0, 12, 50), first=(17, 5))
    off = s.h["offsets"].copy()
    off[20] = off[21] + np.uint64(3)                      # read 19 runs on, read 20 descends
    s2 = Src(ctx, s.h["bases"], 50, 0, off, s.h["quals"], s.h["names"], s.h["name_offsets"])
    text = run_format(s2)
    assert F.span(off, 0, 20)[1] == 0 and text.tobytes().count(b"\n") == 200
    run_format(s2, fmt=FASTA, line_width=7)


def test_generated_names_and_fill(ctx):
    rng = np.random.default_rng(5)
    rl = rng.integers(0, 30, 40)
    reads = [bytes(random_reads(rng, int(n))) for n in rl]
    bases, off = ragged(reads, 1)
    s = Src(ctx, bases, 40, 0, off, None)
    assert run_format(s, name_base=0, use_quals=False).tobytes().startswith(b"@0\n")
    t = run_format(s, name_base=95, use_quals=False, qual_fill=ord("#"), out_shift=6).tobytes()           # 99 -> 100 across the batch
    assert b"@99\n" in t and b"@100\n" in t and b"I" not in t
    t = run_format(s, name_base=2**64 - 3, fmt=FASTA, line_width=8, out_shift=11).tobytes()                # the wrap
    assert t.startswith(b">18446744073709551613\n") and b">18446744073709551615\n" in t and b"\n>0\n" in t and b"\n>36\n" in t
    run_format(s, name_base=10**19 - 20, out_shift=1, use_quals=False)                                        # 19 -> 20 digits
    run_format(s, name_base=999_999_999_999 - 7, fmt=FASTA, use_quals=False)
    # a fill byte with quality bytes absent; 0 and 255 are bytes like any other
    for fill in (0, 255, ord("!")):
        run_format(s, use_quals=False, qual_fill=fill)


@pytest.mark.parametrize("L", [61, 120])
def test_fasta_widths(ctx, L):
    """widths 0, 1, 7, 60, L, L - 1, L + 1 and a divisor of L, on reads of L bases and on ragged reads around them"""
    rng = np.random.default_rng(6 + L)
    rl = [L] * 20 + list(rng.integers(0, 2 * L + 2, 60)) + [0, 1, L - 1, L + 1, 2 * L]
    s = _src(ctx, rng, rl, rng.integers(0, 20, len(rl)), shifts=(1, 0, 3))
    div = 61 if L == 61 else 40
    for i, w in enumerate((0, 1, 7, 60, L, L - 1, L + 1, div, 2**32 - 1)):
        t = run_format(s, fmt=FASTA, line_width=w, out_shift=(3 * i) & 15)
        if w:
            assert max(len(ln) for ln in t.tobytes().split(b"\n")[1::1] if ln[:1] != b">") <= w


# ---------------------------------------------------------------- errors
def test_errors_leave_the_outputs_alone(ctx):
    import torch

    rng = np.random.default_rng(7)
    s = _src(ctx, rng, rng.integers(0, 50, 300), rng.integers(0, 12, 300))
    want_t, _ = s.want(fmt=FASTQ)
    n_bytes = len(want_t)
    f = ctx.lib.kmx_fastx_format
    out = torch.full((n_bytes + GUARD,), SENT, dtype=torch.uint8, device=ctx.device)
    off = torch.full((s.n + 2,), SENT_WORD, dtype=torch.int64, device=ctx.device)
    nb = C.c_uint64(99)

    def call(reads=s.reads, quals=s.d_quals, names=s.names, skip=1, fmt=FASTQ, width=0, fill=73, text=out, room=n_bytes, hn=nb, h=ctx._h):
        return f(h, C.byref(reads) if reads is not None else None, ptr(quals), C.byref(names) if names is not None else None, skip, 0, fmt, width,
                 fill, ptr(text), ptr(off), room, C.byref(hn) if hn is not None else None)

    def untouched():
        return bool((out == SENT).all()) and bool((off == SENT_WORD).all())

    from kmers_amd._lib import Reads

    short = Reads(s.d_names.data_ptr(), s.n - 1, 0, s.d_noff.data_ptr())
    for st in (call(fmt=AUTO), call(fmt=3), call(fmt=FASTQ | SAME_TEXT), call(width=60), call(quals=None, fill=256), call(names=short),
               call(reads=None), call(hn=None), call(h=None)):
        assert st == E_ARG and untouched()
    assert call(quals=None, fill=256, fmt=FASTA, room=10**9) == OK          # FASTA ignores the quality arguments
    out.fill_(SENT), off.fill_(SENT_WORD)
    # the image overlapping a source
    assert call(text=s.d_bases) == E_ARG and call(text=s.d_quals) == E_ARG and call(text=s.d_names) == E_ARG and untouched()
    # one byte too little room: the count is set, nothing is written
    nb.value = 99
    assert call(room=n_bytes - 1) == E_NOMEM and nb.value == n_bytes and untouched()
    # the work buffer's cap: before any kernel runs
    big = 1 << 22
    uniform = Reads(s.d_bases.data_ptr(), big, 0, None)                      # 2^22 empty reads: 32 MiB of record offsets when none are given
    ctx.set_work_buffer_limit(1 << 20)
    try:
        nb.value = 99
        st = f(ctx._h, C.byref(uniform), None, None, 0, 0, FASTQ, 0, 73, ptr(out), None, 1 << 40, C.byref(nb))
        assert st == E_NOMEM and nb.value == 0 and untouched()           # (refused before the count: not for want of room)
    finally:
        ctx.set_work_buffer_limit(0)
    # two calls give identical bytes
    assert call() == OK and nb.value == n_bytes
    first = out.cpu().numpy().copy()
    out.fill_(SENT)
    assert call() == OK and np.array_equal(out.cpu().numpy(), first) and np.array_equal(first[:n_bytes], want_t) and (first[n_bytes:] == SENT).all()


# ---------------------------------------------------------------- round trips and the pipeline
@pytest.mark.parametrize("crlf", [False, True])
def test_round_trip_on_the_device(ctx, crlf):
    """fastq_text -> fastq_records -> fastx_format: the image is the text (with its '\\r' removed); one of the texts spans several
    blocks of the copy and chunks of the parse"""
    rng = np.random.default_rng(8 + crlf)
    layouts = set()
    for n, lo, hi, fixed in ((1, 0, 50, None), (9, 0, 10, None), (3000, 0, 200, None), (500, 0, 0, 150)):
        text = fastq_text(rng, n, lo, hi, crlf=crlf, trail=True, fixed=fixed)
        bases, quals, nr, L, off, names, noff = ctx.fastq_records(ctx.to_device(text))
        assert nr == n
        layouts.add(off is None)
        image, rec = ctx.fastx_format(bases, nr, L, offsets=off, quals=quals, names=names, name_offsets=noff, rec_offsets=True)
        assert image.cpu().numpy().tobytes() == text.replace(b"\r", b"")
        assert image.numel() == int(rec[-1]) and bool((image[rec[:-1]] == ord("@")).all())
    assert layouts == {False, True}          # ragged and uniform reads both went through


def test_pipeline_select_gather_format(ctx, tmp_path):
    """parse, quality filter, gather the names by the index, format -- against the same selection and join on the host"""
    from kmers_amd.api import expected_errors  # noqa: F401  (the rows are the filter's own)

    rng = np.random.default_rng(9)
    n = 2000
    text = fastq_text(rng, n, 0, 120)
    lines = text.split(b"\n")
    bases, quals, nr, L, off, names, noff = ctx.fastq_records(ctx.to_device(text))
    # the filter's survivors, clipped: bases and quality bytes as two batches with one set of offsets and the source index
    kept_b, kept_q, _ = ctx.reads_quality_filter(bases, quals, nr, L, min_q=2, trim_q=12, offsets=off, min_len=20)
    assert 0 < kept_b.n_reads < n and kept_b.index is not None and bool((kept_b.offsets == kept_q.offsets).all())
    kept_n = ctx.reads_gather(names, nr, 0, kept_b.index, offsets=noff)
    image = ctx.fastx_format(kept_b.bases, kept_b.n_reads, 0, offsets=kept_b.offsets, quals=kept_q.bases, names=kept_n.bases, name_offsets=kept_n.offsets)
    hb, hq, ho, hi = kept_b.bases.cpu().numpy().tobytes(), kept_q.bases.cpu().numpy().tobytes(), u64(kept_b.offsets), kept_b.index.cpu().numpy()
    host = b"".join(lines[4 * int(r)] + b"\n" + hb[int(ho[j]):int(ho[j + 1])] + b"\n+\n" + hq[int(ho[j]):int(ho[j + 1])] + b"\n" for j, r in enumerate(hi))
    assert image.cpu().numpy().tobytes() == host
    # a plain selection with the index, as FASTA through write_fastx (a path and a file object)
    keep = ctx.to_device((rng.random(n) < 0.3).astype(np.uint8))
    sel = ctx.reads_select(bases, nr, L, keep=keep, offsets=off, index=True)
    sel_n = ctx.reads_gather(names, nr, 0, sel.index, offsets=noff)
    host = b"".join(b">" + lines[4 * int(r)][1:] + b"\n" + b"".join(lines[4 * int(r) + 1][i:i + 50] + b"\n" for i in range(0, max(len(lines[4 * int(r) + 1]), 1), 50))
                    for r in sel.index.cpu().numpy())
    path = tmp_path / "sel.fa"
    kw = dict(offsets=sel.offsets, names=sel_n.bases, name_offsets=sel_n.offsets, fmt=FASTA, line_width=50)
    assert ctx.write_fastx(str(path), sel.bases, sel.n_reads, 0, **kw) == len(host) and path.read_bytes() == host
    buf = io.BytesIO()
    assert ctx.write_fastx(buf, sel.bases, sel.n_reads, 0, **kw) == len(host) and buf.getvalue() == host


def test_unitigs_write_fasta(ctx):
    """Unitigs.write_fasta against sequences() joined on the host"""
    rng = np.random.default_rng(12)
    k = 21
    genomes = [random_reads(rng, 1500) for _ in range(3)]          # three genomes: at least three unitigs
    reads = np.concatenate([genomes[i % 3][a:a + 100] for i, a in enumerate(rng.integers(0, 1400, 400))])
    kmers, counts = ctx.count_canonical(ctx.to_device(reads), 400, 100, k)
    g = ctx.count_unitigs(kmers, counts, k)
    assert g.n_unitigs > 1
    seq, offs = g.sequences().cpu().numpy().tobytes(), g.offsets.cpu().tolist()
    for width in (60, 0):
        host = b""
        for u in range(g.n_unitigs):
            sq = seq[offs[u] + u * (k - 1):offs[u + 1] + (u + 1) * (k - 1)]
            host += b">%d\n" % u + b"".join(sq[i:i + (width or len(sq))] + b"\n" for i in range(0, len(sq), width or len(sq)))
        buf = io.BytesIO()
        assert g.write_fasta(buf, width=width) == len(host) and buf.getvalue() == host
