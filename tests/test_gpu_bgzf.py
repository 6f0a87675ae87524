"""kmx_bgzf_index and kmx_bgzf_inflate on the GPU (kmx_bgzf.hip), and what the Python layer builds on them (Context.bgzf_index,
bgzf_inflate, load_fastx).

Every comparison is equality with the host reference tests/bgzf_np.py (pinned in tests/test_bgzf_np.py): the index word for word with
the host walk of the chain, the text byte for byte with zlib, the verdict of a corrupted block with zlib plus CRC-32.  There is no
tolerance anywhere.  The raw calls go through run_index / run_inflate, which hand the ABI arrays that are longer than the result and
filled with 0xA5 and look at every byte in front of d_text, behind the text and behind the index words.

The corrupted inputs are malformed data that the call must diagnose; the same flips have gone through the same decoder core under a
sanitizer on the CPU first (tests/test_bgzf_host_decode.py)."""
import ctypes as C
import gzip

import numpy as np
import pytest

from tests import bgzf_np as B
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.fastx_cases import fastq_text
from tests.reads_dev import SENT, SENT_WORD, dev_bytes, ptr

pytestmark = pytest.mark.gpu

OK, E_ARG, E_NOMEM = 0, 1, 6
NO_CRC = 1
GUARD = 64
NONE = 2**64 - 1
FILES = B.files() + B.cut_files()


def _words(ctx, n):
    import torch

    return torch.full((n,), SENT_WORD, dtype=torch.int64, device=ctx.device)


def run_index(ctx, f, shift=0):
    """kmx_bgzf_index through the raw ABI: count-only, then the KMX_E_NOMEM form (nothing written), then into guarded arrays; all
    compared with the host walk -> (d_file, block_offsets, text_offsets, info)"""
    lib = ctx.lib
    bo, to, trailing, has_eof = B.walk(f)
    nb = len(bo) - 1
    d_file = dev_bytes(ctx, np.frombuffer(f, np.uint8), shift)
    info = (C.c_uint64 * 4)()
    assert lib.kmx_bgzf_index(ctx._h, ptr(d_file), len(f), None, None, 0, info) == OK
    want = [nb, int(to[-1]), trailing, has_eof]
    assert list(info) == want
    d_bo, d_to = _words(ctx, nb + 5), _words(ctx, nb + 5)
    if nb:
        info2 = (C.c_uint64 * 4)()
        assert lib.kmx_bgzf_index(ctx._h, ptr(d_file), len(f), ptr(d_bo), ptr(d_to), nb - 1, info2) == E_NOMEM
        assert list(info2) == want
        assert bool((d_bo == SENT_WORD).all()) and bool((d_to == SENT_WORD).all())
    assert lib.kmx_bgzf_index(ctx._h, ptr(d_file), len(f), ptr(d_bo), ptr(d_to), nb + 2, info) == OK
    assert list(info) == want
    got_bo, got_to = d_bo.cpu().numpy().view(np.uint64), d_to.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_bo[:nb + 1], bo) and np.array_equal(got_to[:nb + 1], to)
    assert (d_bo[nb + 1:] == SENT_WORD).all() and (d_to[nb + 1:] == SENT_WORD).all()
    return d_file, d_bo, d_to, want


def run_inflate(ctx, d_file, n_bytes, d_bo, d_to, nb, span, flags=0, want_st=OK):
    """kmx_bgzf_inflate into a text between two 64-byte canaries -> (text bytes, status words, first bad)"""
    import torch

    buf = torch.full((GUARD + span + GUARD,), SENT, dtype=torch.uint8, device=ctx.device)
    status = torch.full((nb + 2,), 0x5A5A5A5A, dtype=torch.int32, device=ctx.device)
    bad = C.c_uint64(7)
    st = ctx.lib.kmx_bgzf_inflate(ctx._h, ptr(d_file), n_bytes, ptr(d_bo), ptr(d_to), nb, flags, C.c_void_p(buf.data_ptr() + GUARD), span,
                                  ptr(status), C.byref(bad))
    assert st == want_st, (st, bad.value)
    h = buf.cpu().numpy()
    assert (h[:GUARD] == SENT).all() and (h[GUARD + span:] == SENT).all()
    hs = status.cpu().numpy()
    assert (hs[nb:] == 0x5A5A5A5A).all()
    return h[GUARD:GUARD + span].tobytes(), hs[:nb], bad.value


@pytest.fixture(scope="module")
def host_texts():
    return {name: B.host_text(f) for name, f in FILES}


@pytest.mark.parametrize("name", [n for n, _ in FILES])
def test_index_and_text_equal_the_host(ctx, host_texts, name):
    f = dict(FILES)[name]
    shift = len(name) % 5                        # the image at any alignment
    d_file, d_bo, d_to, (nb, n_text, _, _) = run_index(ctx, f, shift)
    text, status, bad = run_inflate(ctx, d_file, len(f), d_bo, d_to, nb, n_text)
    assert bad == NONE and not status.any()
    assert text == host_texts[name]
    if not name.startswith("cut_"):
        assert text == gzip.decompress(f)


def test_capacity_and_arguments(ctx):
    import torch

    f = dict(FILES)["concat_eof"]
    d_file, d_bo, d_to, (nb, n_text, _, _) = run_index(ctx, f)
    # a span above the capacity: KMX_E_NOMEM, nothing written
    buf = torch.full((n_text + GUARD,), SENT, dtype=torch.uint8, device=ctx.device)
    status = torch.full((nb,), 0x5A5A5A5A, dtype=torch.int32, device=ctx.device)
    bad = C.c_uint64(7)
    assert ctx.lib.kmx_bgzf_inflate(ctx._h, ptr(d_file), len(f), ptr(d_bo), ptr(d_to), nb, 0, ptr(buf), n_text - 1, ptr(status), C.byref(bad)) == E_NOMEM
    assert bool((buf == SENT).all()) and bool((status == 0x5A5A5A5A).all()) and bad.value == NONE
    # d_text not 16-byte aligned, unknown flags, missing arrays
    assert ctx.lib.kmx_bgzf_inflate(ctx._h, ptr(d_file), len(f), ptr(d_bo), ptr(d_to), nb, 0, C.c_void_p(buf.data_ptr() + 8), n_text, None, None) == E_ARG
    assert ctx.lib.kmx_bgzf_inflate(ctx._h, ptr(d_file), len(f), ptr(d_bo), ptr(d_to), nb, 2, ptr(buf), n_text, None, None) == E_ARG
    assert ctx.lib.kmx_bgzf_inflate(ctx._h, ptr(d_file), len(f), None, ptr(d_to), nb, 0, ptr(buf), n_text, None, None) == E_ARG
    info = (C.c_uint64 * 4)()
    assert ctx.lib.kmx_bgzf_index(ctx._h, ptr(d_file), len(f), ptr(d_bo), None, nb, info) == E_ARG
    assert ctx.lib.kmx_bgzf_index(ctx._h, None, 0, None, None, 0, info) == OK and list(info) == [0, 0, 0, 0]
    # without d_status and h_first_bad
    assert ctx.lib.kmx_bgzf_inflate(ctx._h, ptr(d_file), len(f), ptr(d_bo), ptr(d_to), nb, 0, ptr(buf), n_text, None, None) == OK
    assert buf[:n_text].cpu().numpy().tobytes() == B.host_text(f)


@pytest.mark.parametrize("image", [gzip.compress(b"@r\nACGT\n+\nIIII\n", mtime=0), b"@r\nACGT\n+\nIIII\n", b"\x1f\x8b\x08\x04", B.HEADER[:10] + b"\x0c\0BC\x02\0"
                                   + b"\x27\0" + b"XY\x02\0\0\0" + b"\x03\0" + bytes(8)])
def test_what_is_not_bgzf_is_an_argument_error(ctx, image):
    d_file = dev_bytes(ctx, np.frombuffer(image, np.uint8))
    info = (C.c_uint64 * 4)()
    assert ctx.lib.kmx_bgzf_index(ctx._h, ptr(d_file), len(image), None, None, 0, info) == E_ARG


def test_a_slice_of_blocks_into_a_small_buffer(ctx, host_texts):
    f = dict(FILES)["concat_eof"]
    bo, to, _, _ = B.walk(f)
    d_file, d_bo, d_to, (nb, _, _, _) = run_index(ctx, f)
    i, j = 5, 9
    span = int(to[j] - to[i])
    text, status, bad = run_inflate(ctx, d_file, len(f), d_bo[i:], d_to[i:], j - i, span)
    assert bad == NONE and text == host_texts["concat_eof"][int(to[i]):int(to[j])]
    image = ctx.to_device(f)
    idx = ctx.bgzf_index(image)
    assert (idx.n_blocks, idx.n_text_bytes, idx.trailing, idx.has_eof) == (nb, int(to[-1]), 0, True)
    assert ctx.bgzf_inflate(image, idx, blocks=(i, j)).cpu().numpy().tobytes() == text
    assert ctx.bgzf_inflate(image, idx, blocks=(3, 3)).numel() == 0
    assert ctx.bgzf_inflate(image).cpu().numpy().tobytes() == host_texts["concat_eof"]


def test_crc_flag(ctx, host_texts):
    f = dict(FILES)["concat_eof"]
    bo, to, _, _ = B.walk(f)
    b = 6
    bad_f = B.flipped(f, 8 * (int(bo[b + 1]) - 8) + 3)        # one wrong CRC word
    d_file, d_bo, d_to, (nb, n_text, _, _) = run_index(ctx, bad_f)
    text, status, bad = run_inflate(ctx, d_file, len(f), d_bo, d_to, nb, n_text, flags=NO_CRC)
    assert bad == NONE and not status.any() and text == host_texts["concat_eof"]
    text, status, bad = run_inflate(ctx, d_file, len(f), d_bo, d_to, nb, n_text, want_st=E_ARG)
    assert bad == b and status[b] == 14 and not np.delete(status, b).any() and text == host_texts["concat_eof"]
    with pytest.raises(ValueError, match=f"block {b}.*CRC"):
        ctx.bgzf_inflate(ctx.to_device(bad_f))
    assert ctx.bgzf_inflate(ctx.to_device(bad_f), verify=False).cpu().numpy().tobytes() == host_texts["concat_eof"]


def test_deterministic_across_calls_streams_and_contexts(ctx, host_texts):
    import torch

    from kmers_amd.api import Context

    f = dict(FILES)["concat_eof"]
    image = ctx.to_device(f)
    a = ctx.bgzf_inflate(image).cpu().numpy().tobytes()
    assert ctx.bgzf_inflate(image).cpu().numpy().tobytes() == a == host_texts["concat_eof"]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    c2 = Context(stream=side)
    try:
        with torch.cuda.stream(side):
            assert c2.bgzf_inflate(c2.to_device(f)).cpu().numpy().tobytes() == a
    finally:
        c2.close()
    c3 = Context()
    try:
        assert c3.bgzf_inflate(c3.to_device(f)).cpu().numpy().tobytes() == a
    finally:
        c3.close()


def test_load_fastx_then_records(ctx, tmp_path):
    from kmers_amd.api import bgzf_compress

    rng = np.random.default_rng(8)
    text = fastq_text(rng, 1500, 30, 150)
    f = bgzf_compress(text, 6, 20000)
    assert len(B.walk(f)[0]) > 8
    got = ctx.fastq_records(ctx.load_fastx(f))
    want = ctx.fastq_records(ctx.load_fastx(text))
    for g, w in zip(got, want):
        if hasattr(g, "cpu"):
            assert np.array_equal(g.cpu().numpy(), w.cpu().numpy())
        else:
            assert g == w
    path = tmp_path / "reads.fastq.gz"
    path.write_bytes(f)
    assert ctx.load_fastx(str(path)).cpu().numpy().tobytes() == text
    # write_fastx through bgzf_compress, and back
    bases, quals, n, read_len, offsets, names, noffsets = want
    out = tmp_path / "out.fastq.gz"
    ctx.write_fastx(str(out), bases, n, read_len, offsets=offsets, quals=quals, names=names, name_offsets=noffsets, bgzf_level=6)
    assert gzip.decompress(out.read_bytes()) == text and ctx.load_fastx(str(out)).cpu().numpy().tobytes() == text
    with pytest.raises(ValueError, match="bgzip"):
        ctx.load_fastx(gzip.compress(text))
    with pytest.raises(ValueError, match="behind the last complete"):
        ctx.load_fastx(f[:-5])


def test_single_bit_flips_are_diagnosed(ctx):
    """a three-block file, 200 seeded single-bit flips anywhere in the middle block, inflated with the ORIGINAL index: a status where
    and only where zlib plus CRC-32 say unsound; the neighbours sound and byte-exact; nothing outside the bad block's range touched"""
    f, bo, to, texts = B.three_block_file()
    d_file, d_bo, d_to, (nb, n_text, _, _) = run_index(ctx, f)
    s, e = int(bo[1]), int(bo[2])
    t1, t2 = int(to[1]), int(to[2])
    verdicts = set()
    for bit in B.flip_bits(8 * (e - s), 200, B.FLIP_SEED):
        bad_f = B.flipped(f, 8 * s + bit)
        sound, _ = B.block_verdict(bad_f, s, e, t2 - t1)
        verdicts.add(sound)
        d_bad = dev_bytes(ctx, np.frombuffer(bad_f, np.uint8))
        text, status, bad = run_inflate(ctx, d_bad, len(f), d_bo, d_to, nb, n_text, want_st=OK if sound else E_ARG)
        assert (status[1] == 0) == sound, (bit, status)
        assert status[0] == 0 and status[2] == 0 and bad == (NONE if sound else 1)
        assert text[:t1] == texts[0] and text[t2:] == texts[2], bit
        if sound:
            assert text[t1:t2] == texts[1], bit
    assert verdicts == {True, False}
