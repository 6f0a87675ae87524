"""kmx_fastx_parse_quals on the GPU: the quality lines of a FASTQ image, byte for byte against the line-splitting reference of
tests/quality_np.py, on the texts of tests/fastx_cases.py; the read parse of the same image before and after is unchanged; the
KMX_FASTX_SAME_TEXT forms; the length cross-check; the count-only and KMX_E_NOMEM forms; Context.fastx_quals / fastq_reads."""
import ctypes as C

import numpy as np
import pytest

from tests import quality_np as Q
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import u64
from tests.fastx_cases import EDGE_TEXTS, fastq_text

pytestmark = pytest.mark.gpu

OK, E_ARG, E_NOMEM = 0, 1, 6
FASTQ, FASTA, SAME_TEXT = 1, 2, 0x100
CHUNK = 128 * 1024


def _dev(ctx, text):
    import torch

    return ctx.to_device(text) if len(text) else ctx.empty(0, torch.uint8)


def _check(ctx, orc, text):
    """quality lines == reference; the reads of the same image, parsed before and after, are what the oracle says"""
    d = _dev(ctx, text)
    eb, eo = orc.fastx_parse(text, FASTQ)
    b0, o0 = ctx.fastx_parse(d, FASTQ)
    wq, wo = Q.fastq_quals(text)
    quals, qoff = ctx.fastx_quals(d)
    assert np.array_equal(u64(qoff), wo) and quals.cpu().numpy().tobytes() == wq.tobytes()
    b1, o1 = ctx.fastx_parse(d, FASTQ)
    for b, o in ((b0, o0), (b1, o1)):
        assert np.array_equal(u64(o), eo) and np.array_equal(b.cpu().numpy(), eb)
    # the text's summaries reused after a read parse of the same image (KMX_FASTX_SAME_TEXT): equal results
    q2, qo2 = ctx.fastx_quals(d, same_text=True)
    assert np.array_equal(u64(qo2), wo) and q2.cpu().numpy().tobytes() == wq.tobytes()
    return quals, qoff


def _entry_phases(text):
    """the line number mod 4 at the first byte of every 128 KiB chunk"""
    nl = np.cumsum(np.frombuffer(text, np.uint8) == 10)
    return {int(nl[c - 1]) & 3 for c in range(CHUNK, len(text), CHUNK)}


@pytest.mark.parametrize("i", [i for i, t in enumerate(EDGE_TEXTS) if t[:1] == b"@" or not t])
def test_edge_texts(ctx, orc, i):
    _check(ctx, orc, EDGE_TEXTS[i])


@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("trail", [False, True])
def test_random_fastq(ctx, orc, crlf, trail):
    """'\\r\\n' line ends, quality lines that begin with '@', '>' and '+' (QUAL_ALPHA), a missing final newline; the large text spans
    more than three chunks"""
    rng = np.random.default_rng(41 + 2 * crlf + trail)
    for n, lo, hi in ((1, 0, 50), (9, 0, 10), (3000, 0, 200), (40, 3000, 9000)):
        text = fastq_text(rng, n, lo, hi, crlf=crlf, trail=trail)
        quals, qoff = _check(ctx, orc, text)
        if n == 3000:
            assert len(text) > 3 * CHUNK and len(_entry_phases(text)) >= 2
            first = quals.cpu().numpy()[u64(qoff)[:-1][np.diff(u64(qoff).astype(np.int64)) > 0].astype(np.int64)]
            assert {ord("@"), ord(">"), ord("+")} <= set(first.tolist())


def test_chunks_entered_in_every_phase(ctx, orc):
    """line lengths chosen so that the first four chunk boundaries fall inside a header, a sequence, a quality and a '+' line"""
    from tests.fastx_cases import QUAL_ALPHA

    rng = np.random.default_rng(42)
    seq = bytes(rng.choice(list(b"ACGT"), CHUNK).astype(np.uint8))
    qual = bytes(rng.choice(QUAL_ALPHA, CHUNK).astype(np.uint8))
    lines = [b"@" + b"h" * (3 * CHUNK // 2), b"AC", b"+", b"#@",      # boundary 1 inside the header
             b"@r1", seq, b"+", qual,                                  # boundaries 2 and 3 inside the sequence and the quality line
             b"@r2", b"ACGT", b"+" + b"r" * CHUNK, b"@>+I"]            # boundary 4 inside the '+' line
    text = b"\n".join(lines) + b"\n" + fastq_text(rng, 200)
    assert len(text) > 3 * CHUNK and _entry_phases(text) == {0, 1, 2, 3}
    _check(ctx, orc, text)


def test_truncated_last_record(ctx, orc):
    rng = np.random.default_rng(43)
    full = fastq_text(rng, 50, 10, 80)
    lines = full.split(b"\n")
    for cut in (b"\n".join(lines[:-2]), b"\n".join(lines[:-2]) + b"\n", b"\n".join(lines[:-3]) + b"\n", b"\n".join(lines[:-4]),
                full[:-1], full[:-7]):
        _check(ctx, orc, cut)
    # a record without its quality line: one quality line fewer than reads, and fastq_reads says so
    cut = b"\n".join(lines[:-2]) + b"\n"
    assert len(Q.fastq_quals(cut)[1]) == len(orc.fastx_parse(cut, FASTQ)[1]) - 1
    with pytest.raises(ValueError, match="49 quality lines for 50 reads"):
        ctx.fastq_reads(_dev(ctx, cut))


def test_mismatch_is_reported(ctx, orc):
    rng = np.random.default_rng(44)
    lines = fastq_text(rng, 3000, 20, 60).split(b"\n")
    d = _dev(ctx, b"\n".join(lines))
    bases, quals, n, L, off = ctx.fastq_reads(d)
    assert n == 3000 and quals.numel() == bases.numel()
    for r in (2999, 1234, 7):                       # the smallest planted read is reported
        lines[4 * r + 3] = lines[4 * r + 3] + b"I"
        d = _dev(ctx, b"\n".join(lines))
        with pytest.raises(ValueError, match=f"read {r}:"):
            ctx.fastq_reads(d)
        _, offsets = ctx.fastx_parse(d, FASTQ)
        bad, nr = C.c_uint64(0), C.c_uint64(0)
        q = ctx.empty(d.numel(), __import__("torch").uint8)
        qo = ctx.empty(3001, __import__("torch").int64)
        st = ctx.lib.kmx_fastx_parse_quals(ctx._h, C.c_void_p(d.data_ptr()), d.numel(), FASTQ, C.c_void_p(q.data_ptr()), C.c_void_p(qo.data_ptr()),
                                           3000, C.c_void_p(offsets.data_ptr()), C.byref(nr), None, C.byref(bad))
        assert st == OK and bad.value == r == Q.first_mismatch(u64(qo), u64(offsets))


def test_formats_counts_and_room(ctx):
    import torch

    f = ctx.lib.kmx_fastx_parse_quals
    rng = np.random.default_rng(45)
    text = fastq_text(rng, 5000, 20, 200)
    wq, wo = Q.fastq_quals(text)
    d = _dev(ctx, text)
    nr, nb = C.c_uint64(7), C.c_uint64(7)
    tp, n = C.c_void_p(d.data_ptr()), d.numel()
    assert f(ctx._h, tp, n, FASTQ, None, None, 0, None, C.byref(nr), C.byref(nb), None) == OK          # count only
    assert (nr.value, nb.value) == (len(wo) - 1, len(wq))
    assert f(ctx._h, tp, n, 0, None, None, 0, None, C.byref(nr), C.byref(nb), None) == OK               # KMX_FASTX_AUTO
    assert f(ctx._h, tp, n, FASTA, None, None, 0, None, C.byref(nr), C.byref(nb), None) == E_ARG
    fa = _dev(ctx, b">x\nACGT\n")
    assert f(ctx._h, C.c_void_p(fa.data_ptr()), fa.numel(), 0, None, None, 0, None, C.byref(nr), C.byref(nb), None) == E_ARG
    assert f(ctx._h, C.c_void_p(fa.data_ptr()), fa.numel(), FASTQ, None, None, 0, None, C.byref(nr), C.byref(nb), None) == E_ARG
    q = torch.full((len(text) + 64,), 0x5A, dtype=torch.uint8, device=ctx.device)
    qo = torch.full((1000 + 1 + 64,), -1, dtype=torch.int64, device=ctx.device)
    qp, op = C.c_void_p(q.data_ptr()), C.c_void_p(qo.data_ptr())
    assert f(ctx._h, tp, n, FASTQ, qp, None, 1000, None, C.byref(nr), C.byref(nb), None) == E_ARG       # one output without the other
    assert f(ctx._h, tp, n, FASTQ, qp, op, 1000, None, C.byref(nr), C.byref(nb), None) == E_NOMEM
    assert (nr.value, nb.value) == (len(wo) - 1, len(wq)) and bool((qo == -1).all()) and bool((q == 0x5A).all())   # nothing written
    qo = torch.full((5000 + 1 + 64,), -1, dtype=torch.int64, device=ctx.device)
    assert f(ctx._h, tp, n, FASTQ | SAME_TEXT, qp, C.c_void_p(qo.data_ptr()), 5000, None, C.byref(nr), C.byref(nb), None) == OK
    assert np.array_equal(u64(qo)[:5001], wo) and bool((qo[5001:] == -1).all())
    got = q.cpu().numpy()
    assert got[:len(wq)].tobytes() == wq.tobytes() and (got[len(wq):] == 0x5A).all()
    assert f(None, tp, n, FASTQ, None, None, 0, None, C.byref(nr), C.byref(nb), None) == E_ARG


def test_fastq_reads_layouts(ctx):
    rng = np.random.default_rng(46)
    text = fastq_text(rng, 300, fixed=75)
    bases, quals, n, L, off = ctx.fastq_reads(_dev(ctx, text))
    assert (n, L, off) == (300, 75, None) and quals.cpu().numpy().tobytes() == Q.fastq_quals(text)[0].tobytes()
    text = fastq_text(rng, 300, 0, 90)
    bases, quals, n, L, off = ctx.fastq_reads(_dev(ctx, text))
    assert n == 300 and off is not None and np.array_equal(u64(off), Q.fastq_quals(text)[1])
    masked, rows = ctx.reads_quality(bases, quals, n, L, min_q=3, trim_q=20, k=5, offsets=off)
    want = Q.reads_quality_np(bases.cpu().numpy(), quals.cpu().numpy(), n, 0, u64(off), 33, 3, 20, 5)
    assert (u64(rows) == want[1]).all() and masked.cpu().numpy().tobytes() == want[0].tobytes()
