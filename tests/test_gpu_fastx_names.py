"""kmx_fastx_parse_names on the GPU: line 0 of every record of a FASTQ image, byte for byte against the line-splitting reference of
tests/fastx_out_np.py, on the texts of tests/fastx_cases.py; the read and the quality parse of the same image before and after are
unchanged; the KMX_FASTX_SAME_TEXT forms behind either of them; every truncation of the last record; the count-only and KMX_E_NOMEM
forms; Context.fastx_names / fastq_records."""
import ctypes as C

import numpy as np
import pytest

from tests import fastx_out_np as F
from tests import quality_np as Q
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import u64
from tests.fastx_cases import EDGE_TEXTS, QUAL_ALPHA, fastq_text

pytestmark = pytest.mark.gpu

OK, E_ARG, E_NOMEM = 0, 1, 6
FASTQ, FASTA, SAME_TEXT = 1, 2, 0x100
CHUNK = 128 * 1024


def _dev(ctx, text):
    import torch

    return ctx.to_device(text) if len(text) else ctx.empty(0, torch.uint8)


def _same(names, noff, want):
    return np.array_equal(u64(noff), want[1]) and names.cpu().numpy().tobytes() == want[0].tobytes()


def _check(ctx, orc, text):
    """names == reference, alone and behind a read parse and a quality parse of the same image (KMX_FASTX_SAME_TEXT); the reads and
    the quality lines of the image, parsed before and after the names, are what their references say"""
    d = _dev(ctx, text)
    want = F.fastq_names(text)
    eb, eo = orc.fastx_parse(text, FASTQ)
    wq, wo = Q.fastq_quals(text)

    def reads_and_quals_unchanged():
        b, o = ctx.fastx_parse(d, FASTQ)
        assert np.array_equal(u64(o), eo) and np.array_equal(b.cpu().numpy(), eb)
        q, qo = ctx.fastx_quals(d)
        assert np.array_equal(u64(qo), wo) and q.cpu().numpy().tobytes() == wq.tobytes()

    reads_and_quals_unchanged()
    names, noff = ctx.fastx_names(d)
    assert _same(names, noff, want)
    reads_and_quals_unchanged()
    ctx.fastx_parse(d, FASTQ)
    assert _same(*ctx.fastx_names(d, same_text=True), want), "behind a read parse"
    ctx.fastx_quals(d)
    assert _same(*ctx.fastx_names(d, same_text=True), want), "behind a quality parse"
    q, qo = ctx.fastx_quals(d, same_text=True)
    assert np.array_equal(u64(qo), wo) and q.cpu().numpy().tobytes() == wq.tobytes(), "a quality parse behind the names"
    return names, noff


def _entry_phases(text):
    """the line number mod 4 at the first byte of every 128 KiB chunk"""
    nl = np.cumsum(np.frombuffer(text, np.uint8) == 10)
    return {int(nl[c - 1]) & 3 for c in range(CHUNK, len(text), CHUNK)}


@pytest.mark.parametrize("i", [i for i, t in enumerate(EDGE_TEXTS) if t[:1] == b"@" or not t])
def test_edge_texts(ctx, orc, i):
    """among them the 70 000-byte header and 3000 records of six bytes"""
    _check(ctx, orc, EDGE_TEXTS[i])


@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("trail", [False, True])
def test_random_fastq(ctx, orc, crlf, trail):
    """'\\r\\n' line ends, a missing final newline; the large text spans more than three chunks"""
    rng = np.random.default_rng(41 + 2 * crlf + trail)
    for n, lo, hi in ((1, 0, 50), (9, 0, 10), (3000, 0, 200), (40, 3000, 9000)):
        text = fastq_text(rng, n, lo, hi, crlf=crlf, trail=trail)
        names, noff = _check(ctx, orc, text)
        assert noff.numel() == n + 1
        if n == 3000:
            assert len(text) > 3 * CHUNK and len(_entry_phases(text)) >= 2


def test_chunks_entered_in_every_phase(ctx, orc):
    """line lengths chosen so that the first four chunk boundaries fall inside a header, a sequence, a quality and a '+' line"""
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
    """every truncation of the last record, and how many names the reference finds in each"""
    rng = np.random.default_rng(43)
    full = fastq_text(rng, 50, 10, 80)
    lines = full.split(b"\n")          # 200 lines and the empty piece behind the last newline
    head = b"\n".join(lines[:196]) + b"\n"
    cuts = [(full, 50), (full[:-1], 50), (full[:-7], 50),                                 # the whole text; inside the last quality line
            (b"\n".join(lines[:-2]), 50), (b"\n".join(lines[:-2]) + b"\n", 50),          # before the quality line, with and without '+\n'
            (b"\n".join(lines[:-3]) + b"\n", 50), (b"\n".join(lines[:-4]), 50),          # behind the sequence; behind the header, no newline
            (head + lines[196][:3], 50), (head + b"@", 50), (head, 49),                   # inside the header; its first byte; no record 49
            (head + b"\n", 50), (head[:-1], 49)]                                          # an empty header line; record 48 without its last newline
    for cut, n_names in cuts:
        assert len(F.fastq_names(cut)[1]) - 1 == n_names
        _, noff = _check(ctx, orc, cut)
        assert noff.numel() - 1 == n_names
    # a record with nothing but its header: one name more than reads, and fastq_records says so
    cut = head + b"@last"
    assert len(F.fastq_names(cut)[1]) - 1 == len(orc.fastx_parse(cut, FASTQ)[1]) - 1 + 1
    with pytest.raises(ValueError, match="50 names for 49 reads"):
        ctx.fastq_records(_dev(ctx, cut))


def test_formats_counts_and_room(ctx):
    import torch

    f = ctx.lib.kmx_fastx_parse_names
    rng = np.random.default_rng(45)
    text = fastq_text(rng, 5000, 20, 200)
    wn, wo = F.fastq_names(text)
    d = _dev(ctx, text)
    nr, nb = C.c_uint64(7), C.c_uint64(7)
    tp, n = C.c_void_p(d.data_ptr()), d.numel()
    assert f(ctx._h, tp, n, FASTQ, None, None, 0, C.byref(nr), C.byref(nb)) == OK          # count only
    assert (nr.value, nb.value) == (len(wo) - 1, len(wn))
    assert f(ctx._h, tp, n, 0, None, None, 0, C.byref(nr), C.byref(nb)) == OK               # KMX_FASTX_AUTO
    assert (nr.value, nb.value) == (len(wo) - 1, len(wn))
    assert f(ctx._h, tp, n, FASTA, None, None, 0, C.byref(nr), C.byref(nb)) == E_ARG
    fa = _dev(ctx, b">x\nACGT\n")
    assert f(ctx._h, C.c_void_p(fa.data_ptr()), fa.numel(), 0, None, None, 0, C.byref(nr), C.byref(nb)) == E_ARG
    assert f(ctx._h, C.c_void_p(fa.data_ptr()), fa.numel(), FASTQ, None, None, 0, C.byref(nr), C.byref(nb)) == E_ARG
    assert f(ctx._h, C.c_void_p(d.data_ptr() + 1), n - 1, FASTQ, None, None, 0, C.byref(nr), C.byref(nb)) == E_ARG   # d_text not 16-byte aligned
    q = torch.full((len(text) + 64,), 0x5A, dtype=torch.uint8, device=ctx.device)
    qo = torch.full((1000 + 1 + 64,), -1, dtype=torch.int64, device=ctx.device)
    qp, op = C.c_void_p(q.data_ptr()), C.c_void_p(qo.data_ptr())
    assert f(ctx._h, tp, n, FASTQ, qp, None, 1000, C.byref(nr), C.byref(nb)) == E_ARG       # one output without the other
    assert f(ctx._h, tp, n, FASTQ, qp, op, 1000, C.byref(nr), C.byref(nb)) == E_NOMEM
    assert (nr.value, nb.value) == (len(wo) - 1, len(wn)) and bool((qo == -1).all()) and bool((q == 0x5A).all())   # nothing written
    qo = torch.full((5000 + 1 + 64,), -1, dtype=torch.int64, device=ctx.device)
    assert f(ctx._h, tp, n, FASTQ | SAME_TEXT, qp, C.c_void_p(qo.data_ptr()), 5000, C.byref(nr), C.byref(nb)) == OK
    assert np.array_equal(u64(qo)[:5001], wo) and bool((qo[5001:] == -1).all())
    got = q.cpu().numpy()
    assert got[:len(wn)].tobytes() == wn.tobytes() and (got[len(wn):] == 0x5A).all()
    assert f(None, tp, n, FASTQ, None, None, 0, C.byref(nr), C.byref(nb)) == E_ARG


def test_fastq_records_and_gather(ctx):
    """fastq_records: the names beside the reads of fastq_reads; the names are a ragged batch that reads_gather reorders"""
    rng = np.random.default_rng(46)
    text = fastq_text(rng, 300, 0, 90)
    bases, quals, n, L, off, names, noff = ctx.fastq_records(_dev(ctx, text))
    wn, wo = F.fastq_names(text)
    assert n == 300 and _same(names, noff, (wn, wo)) and quals.cpu().numpy().tobytes() == Q.fastq_quals(text)[0].tobytes()
    index = rng.permutation(300)[:77].astype(np.int64)
    g = ctx.reads_gather(names, n, 0, ctx.to_device(index), offsets=noff)
    host = [wn.tobytes()[int(wo[i]):int(wo[i + 1])] for i in index]
    assert g.bases.cpu().numpy().tobytes() == b"".join(host) and np.array_equal(np.diff(u64(g.offsets).astype(np.int64)), [len(x) for x in host])
