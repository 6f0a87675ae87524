"""kmx_bgzf_deflate on the GPU (kmx_bgzf.hip), and what the Python and C++ layers build on it (Context.bgzf_deflate,
write_fastx(bgzf_device=True), kmx::naive_impl::bgzf_deflate).

Every comparison is equality.  The device's image is held byte for byte to the host model's (tests/cpp/bgzf_encode_check.cpp,
compiled here; held to zlib on the CPU by tests/test_bgzf_host_encode.py), and once more to zlib itself: gzip's text, the host walk's
offsets, the device's own inflate with CRC.  The raw call goes through run_deflate, which hands in a file buffer longer than the
image and filled with 0xA5 and looks at every byte in front of the image and behind it."""
import ctypes as C
import gzip
import io
import os
import subprocess

import numpy as np
import pytest

from tests import bgzf_deflate_cases as K
from tests import bgzf_np as B
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.reads_dev import SENT, SENT_WORD, dev_bytes, ptr

pytestmark = pytest.mark.gpu

OK, E_ARG, E_NOMEM = 0, 1, 6
GUARD = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (65280, 9000)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bgzf_deflate")
    exe, _ = K.compile_host(tmp)
    ents = K.entries(SIZES)
    return exe, ents, K.host_images(exe, ents, tmp)


def run_deflate(ctx, text, bb, flags=0, shift_text=0, shift_file=0, slack=100, offsets=True):
    """kmx_bgzf_deflate through the raw ABI into a guarded buffer of the image's size + slack -> (image bytes, offsets or None, info);
    the bytes in front of d_file and behind the image, up to file_capacity and past it, must be untouched"""
    import torch

    lib = ctx.lib
    d_text = dev_bytes(ctx, np.frombuffer(text, np.uint8), shift_text)
    info = (C.c_uint64 * 4)()
    assert lib.kmx_bgzf_deflate(ctx._h, ptr(d_text) if text else None, len(text), bb, flags, None, 0, None, info) == OK
    size = int(info[1])
    n_pieces = (len(text) + bb - 1) // bb
    assert info[0] == n_pieces + 1 and info[3] == len(text) and size <= lib.kmx_bgzf_deflate_bound(len(text), bb) == K.bound(len(text), bb)
    buf = torch.full((GUARD + shift_file + size + slack + GUARD,), SENT, dtype=torch.uint8, device=ctx.device)
    assert buf.data_ptr() % 256 == 0
    d_file = buf[GUARD + shift_file:]
    d_off = torch.full((n_pieces + 2 + 3,), SENT_WORD, dtype=torch.int64, device=ctx.device) if offsets else None
    info2 = (C.c_uint64 * 4)()
    assert lib.kmx_bgzf_deflate(ctx._h, ptr(d_text) if text else None, len(text), bb, flags, ptr(d_file), size + slack, ptr(d_off), info2) == OK
    assert list(info2) == list(info)
    got = buf.cpu().numpy()
    at = GUARD + shift_file
    assert (got[:at] == SENT).all() and (got[at + size:] == SENT).all()
    off = None
    if offsets:
        off = d_off.cpu().numpy()
        assert (off[n_pieces + 2:] == SENT_WORD).all()
        off = off[:n_pieces + 2].view(np.uint64)
    return got[at:at + size].tobytes(), off, list(info)


def test_device_image_is_the_host_models(ctx, model):
    _, ents, images = model
    for (name, bb, _, text), (want, n_stored, _) in zip(ents, images):
        got, off, info = run_deflate(ctx, text, bb)
        assert got == want, name
        assert gzip.decompress(got) == text, name
        bo, to, trailing, has_eof = B.walk(got)
        assert trailing == 0 and has_eof == 1 and np.array_equal(off, bo), name
        assert info == [len(bo) - 1, len(got), n_stored, len(text)], name
        if text:
            assert ctx.bgzf_inflate(ctx.to_device(got), verify=True).cpu().numpy().tobytes() == text, name


def test_sizes_on_the_device(ctx, model):
    """the two size conditions and the ratio bound of tests/test_bgzf_host_encode.py, on the device's own bytes"""
    _, ents, _ = model
    by = {name: text for name, _, _, text in ents}
    c = ctx.bgzf_deflate(ctx.to_device(by["c_one_byte@65280"]))
    assert int(c.numel()) < 1024
    for name in ("e_fastq", "f_illumina"):
        text = by[name + "@65280"]
        n = int(ctx.bgzf_deflate(ctx.to_device(text)).numel())
        l1 = len(B.write(text, 1, 65280))
        print(f"{name}: image {n}, Z_HUFFMAN_ONLY {K.huffman_only_size(text)}, level 1 {l1} ({n / l1:.4f})")
        assert n <= K.huffman_only_size(text) and n <= K.RATIO_BOUND_L1[name] * l1, name


def test_many_small_blocks_with_and_without_a_capped_work_buffer(ctx, model, tmp_path):
    """256-byte blocks over 2 MiB: 8192 blocks -- more than one launch of waves, and with the work buffer capped more than one chunk of
    slots (the pieces are then coded twice: once for the size, once for the bytes).  The bytes are the same, and the host model's."""
    exe, _, _ = model
    rng = np.random.default_rng(5)
    text = K.illumina_text(rng, n_reads=6200)[:2 << 20]
    assert len(text) == 2 << 20
    a, off, info = run_deflate(ctx, text, 256)
    assert info[0] == 8193 and gzip.decompress(a) == text and np.array_equal(off, B.walk(a)[0])
    assert a == K.host_images(exe, [("small_blocks", 256, 0, text)], tmp_path, "small")[0][0]
    lib = ctx.lib
    d_text = ctx.to_device(text)
    try:
        ctx.set_work_buffer_limit(1 << 20)       # 8194 * 16 bytes of per-block words, and slots of 512 bytes for some 1700 pieces
        b, off_b, info_b = run_deflate(ctx, text, 256)
        assert b == a and info_b == info and np.array_equal(off_b, off)
        ctx.set_work_buffer_limit(100 << 10)     # not even the per-block words
        out = (C.c_uint64 * 4)()
        assert lib.kmx_bgzf_deflate(ctx._h, ptr(d_text), len(text), 256, 0, None, 0, None, out) == E_NOMEM
        # the per-block words of 33 blocks of 65280 (1 KiB) fit, not one slot of 64 KiB behind them: refused; stored blocks need no
        # slot, and no text needs none either -- the marker alone comes out under the same cap
        ctx.set_work_buffer_limit(32 << 10)
        assert lib.kmx_bgzf_deflate(ctx._h, ptr(d_text), len(text), 65280, 0, None, 0, None, out) == E_NOMEM
        assert lib.kmx_bgzf_deflate(ctx._h, ptr(d_text), len(text), 65280, K.STORED, None, 0, None, out) == OK
        assert list(out) == [34, K.bound(len(text), 65280), 33, len(text)]
        assert run_deflate(ctx, b"", 65280)[0] == B.EOF_MARKER
    finally:
        ctx.set_work_buffer_limit(0)
    c, _, _ = run_deflate(ctx, text, 256)
    assert c == a


def test_any_alignment(ctx, model):
    _, ents, images = model
    by = {name: (bb, text, img[0]) for (name, bb, _, text), img in zip(ents, images)}
    for name in ("f_illumina@9000", "d_random@65280", "h_match_then_3@65280"):
        bb, text, want = by[name]
        for shift in (1, 2, 3):
            assert run_deflate(ctx, text, bb, shift_text=shift, shift_file=shift)[0] == want, (name, shift)
            assert run_deflate(ctx, text, bb, shift_text=3 - shift, shift_file=shift + 4, slack=0)[0] == want, (name, shift)


def test_capacity_one_byte_short_writes_nothing(ctx, model):
    import torch

    _, ents, images = model
    name, bb, _, text = ents[[e[0] for e in ents].index("f_illumina@9000")]
    want = images[[e[0] for e in ents].index("f_illumina@9000")][0]
    d_text = ctx.to_device(text)
    d_file = torch.full((len(want) + 64,), SENT, dtype=torch.uint8, device=ctx.device)
    d_off = torch.full((len(text) // bb + 8,), SENT_WORD, dtype=torch.int64, device=ctx.device)
    info = (C.c_uint64 * 4)()
    assert ctx.lib.kmx_bgzf_deflate(ctx._h, ptr(d_text), len(text), bb, 0, ptr(d_file), len(want) - 1, ptr(d_off), info) == E_NOMEM
    assert list(info)[:2] == [(len(text) + bb - 1) // bb + 1, len(want)] and info[3] == len(text)
    assert bool((d_file == SENT).all()) and bool((d_off == SENT_WORD).all())
    assert ctx.lib.kmx_bgzf_deflate(ctx._h, ptr(d_text), len(text), bb, 0, ptr(d_file), len(want), None, info) == OK
    assert d_file.cpu().numpy()[:len(want)].tobytes() == want and bool((d_file[len(want):] == SENT).all())


def test_arguments(ctx):
    info = (C.c_uint64 * 4)()
    d = ctx.to_device(b"ACGT")
    lib = ctx.lib
    assert lib.kmx_bgzf_deflate(ctx._h, ptr(d), 4, 65281, 0, None, 0, None, info) == E_ARG
    assert lib.kmx_bgzf_deflate(ctx._h, ptr(d), 4, 0, 2, None, 0, None, info) == E_ARG
    assert lib.kmx_bgzf_deflate(ctx._h, None, 4, 0, 0, None, 0, None, info) == E_ARG
    assert lib.kmx_bgzf_deflate(ctx._h, ptr(d), 4, 0, 0, None, 0, None, None) == E_ARG
    assert lib.kmx_bgzf_deflate(ctx._h, ptr(d), 4, 0, 0, None, 0, None, info) == OK and list(info) == [2, 18 + 9 + 8 + 28, 1, 4]
    with pytest.raises(ValueError):
        ctx.bgzf_deflate(d, block_bytes=0)


def test_stored_flag_is_bgzf_compress_level_0(ctx, model):
    from kmers_amd.api import bgzf_compress

    _, ents, _ = model
    for name, bb, _, text in ents:
        if name.split("_")[0] not in "abdg":
            continue
        got, off, info = run_deflate(ctx, text, bb, flags=K.STORED)
        assert got == bgzf_compress(text, 0, bb), name
        assert info[2] == info[0] - 1 and np.array_equal(off, B.walk(got)[0])
        assert ctx.bgzf_deflate(ctx.to_device(text), bb, stored=True).cpu().numpy().tobytes() == got


def test_same_bytes_across_calls_streams_and_contexts(ctx, model):
    import torch

    from kmers_amd.api import Context

    _, ents, images = model
    i = [e[0] for e in ents].index("f_illumina@9000")
    text, want = ents[i][3], images[i][0]
    for _ in range(2):
        img, off = ctx.bgzf_deflate(ctx.to_device(text), 9000, offsets=True)
        assert img.cpu().numpy().tobytes() == want
        assert np.array_equal(off.cpu().numpy().view(np.uint64), B.walk(want)[0])
    side = torch.cuda.Stream(device=ctx.device)
    c2 = Context(stream=side)
    try:
        assert c2.bgzf_deflate(c2.to_device(text), 9000).cpu().numpy().tobytes() == want
    finally:
        c2.close()
    c3 = Context()
    try:
        assert c3.bgzf_deflate(c3.to_device(text), 9000).cpu().numpy().tobytes() == want
    finally:
        c3.close()


def test_write_fastx_on_the_device(ctx):
    from tests.fastx_cases import fastq_text

    text = fastq_text(np.random.default_rng(8), 1500, 30, 150)
    want = ctx.fastq_records(ctx.load_fastx(text))
    bases, quals, n, read_len, offsets, names, noffsets = want
    kw = dict(offsets=offsets, quals=quals, names=names, name_offsets=noffsets)
    plain, gz, gz0 = io.BytesIO(), io.BytesIO(), io.BytesIO()
    ctx.write_fastx(plain, bases, n, read_len, **kw)
    assert ctx.write_fastx(gz, bases, n, read_len, bgzf_device=True, **kw) == len(gz.getvalue())
    assert gzip.decompress(gz.getvalue()) == plain.getvalue() == text
    assert len(gz.getvalue()) < 0.6 * len(text)
    got = ctx.fastq_records(ctx.load_fastx(gz.getvalue()))
    for g, w in zip(got, want):
        if hasattr(g, "cpu"):
            assert np.array_equal(g.cpu().numpy(), w.cpu().numpy())
        else:
            assert g == w
    with pytest.raises(ValueError, match="no compression levels"):
        ctx.write_fastx(io.BytesIO(), bases, n, read_len, bgzf_device=True, bgzf_level=6, **kw)
    ctx.write_fastx(gz0, bases, n, read_len, bgzf_device=True, bgzf_level=0, **kw)
    host0 = io.BytesIO()
    ctx.write_fastx(host0, bases, n, read_len, bgzf_level=0, **kw)
    assert gz0.getvalue() == host0.getvalue()


def test_cpp_bgzf_deflate_on_gpu(tmp_path, model):
    _, ents, images = model
    i = [e[0] for e in ents].index("f_illumina@9000")
    lib = os.path.join(ROOT, "kmers_amd", "libkmx.so")
    assert os.path.exists(lib), "build libkmx.so first (python -m kmers_amd.build)"
    exe = str(tmp_path / "test_bgzf_deflate_hpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_bgzf_deflate_hpp.cpp"),
                           "-L", os.path.join(ROOT, "kmers_amd"), "-lkmx", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "kmers_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    paths = [tmp_path / "t.fastq", tmp_path / "want.gz", tmp_path / "stored.gz"]
    paths[0].write_bytes(ents[i][3])
    paths[1].write_bytes(images[i][0])
    paths[2].write_bytes(B.write(ents[i][3], 0, 9000))
    r = subprocess.run([exe] + [str(p) for p in paths], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all C++ BGZF deflate checks passed" in r.stdout
