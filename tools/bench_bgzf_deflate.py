"""dev tool: kmx_bgzf_deflate beside the host path it replaces (write_fastx(..., bgzf_level=...): the text copied to the host and
compressed there by zlib) and beside a plain copy; one process, so that all versions see the same device state.  The device's image
is checked first: it must inflate to the text, on the host (zlib, every block) and on the device (kmx_bgzf_inflate with CRC).
  input    tools/bench_bgzf.make_text: a FASTQ image of n reads of 150 bp
  deflate  kmx_bgzf_deflate into a buffer that is there (of kmx_bgzf_deflate_bound bytes), and the same plus the device-to-host copy
           of the image: the .gz file in host memory
  stored   the same call with KMX_BGZF_DEFLATE_STORED: CRC, scan and copy kernel alone -- what the coding kernel adds is the difference
  (a) host the device-to-host copy of the text plus bgzf_compress at levels 1 and 6 over at most 16 threads (zlib releases the GIL):
           what write_fastx does today
  (b) copy Tensor.copy_ of the text's bytes on the device: the floor of anything that reads the text
  inflate  kmx_bgzf_inflate of the device's image into a buffer that is there, with the CRC-32 kernel, for scale
Times are medians of synchronised runs (ms, wall clock between two synchronises), the versions alternating, after two warm-up calls
of each; GB/s = bytes of text / time.
Output: profiles/bgzf_deflate_bench.txt.
  python tools/bench_bgzf_deflate.py [n_reads, default 2e6] [reps, default 5]"""
import ctypes as C
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tools.bench_bgzf import THREADS, make_text, medians


def host_compress(text, level):
    from kmers_amd.api import BGZF_EOF, bgzf_compress

    step = 65280 * 64
    with ThreadPoolExecutor(THREADS) as ex:
        parts = list(ex.map(lambda i: bgzf_compress(memoryview(text)[i:i + step], level)[:-28], range(0, len(text), step)))
    return b"".join(parts) + BGZF_EOF


def host_inflate(f):
    p, jobs = 0, []
    while p < len(f):
        size = int.from_bytes(f[p + 16:p + 18], "little") + 1
        jobs.append((p + 18, p + size - 8))
        p += size
    with ThreadPoolExecutor(THREADS) as ex:
        return b"".join(ex.map(lambda j: zlib.decompress(memoryview(f)[j[0]:j[1]], -15), jobs, chunksize=64))


def main():
    from kmers_amd import _lib
    from kmers_amd.api import Context, _ptr

    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 2_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    t0 = time.perf_counter()
    text = make_text(n)
    nt = len(text)
    print(f"bgzf deflate: {n:.0e} FASTQ reads of 150 bp, {nt:.3e} bytes of text; built in {time.perf_counter() - t0:.1f} s by {THREADS} threads; "
          f"median of {reps} alternating runs each (ms) after 2 warm-up calls; GB/s = bytes of text / time; MI355X")
    ctx = Context(0)
    sync = torch.cuda.synchronize
    d_text = ctx.to_device(text)
    image, off = ctx.bgzf_deflate(d_text, offsets=True)
    f = image.cpu().numpy().tobytes()
    if host_inflate(f) != text:
        print("MISMATCH: zlib does not inflate the device's image to the text; not timed")
        return 1
    if ctx.bgzf_inflate(image).cpu().numpy().tobytes() != text:
        print("MISMATCH: the device does not inflate its own image to the text; not timed")
        return 1
    sizes = {lv: len(host_compress(text, lv)) for lv in (1, 6)}
    nb = int(off.numel()) - 1
    print(f"{nb} blocks; the image inflates to the text on the host and on the device.  bytes: device {len(f)} ({len(f) / nt:.4f} of the text), "
          f"zlib level 1 {sizes[1]} ({len(f) / sizes[1]:.4f}), level 6 {sizes[6]} ({len(f) / sizes[6]:.4f})")
    room = int(ctx.lib.kmx_bgzf_deflate_bound(nt, 65280))
    buf = torch.empty(room, dtype=torch.uint8, device=ctx.device)
    dst = torch.empty(nt, dtype=torch.uint8, device=ctx.device)
    info = (C.c_uint64 * 4)()
    idx = ctx.bgzf_index(image)

    def deflate(flags=0):
        ctx._ck(ctx.lib.kmx_bgzf_deflate(ctx._h, _ptr(d_text), nt, 65280, flags, _ptr(buf), room, None, info))
        return int(info[1])

    got = torch.empty(nt, dtype=torch.uint8, device=ctx.device)
    status = torch.zeros(idx.n_blocks, dtype=torch.int32, device=ctx.device)
    bad = C.c_uint64(0)

    def inflate():
        ctx._ck(ctx.lib.kmx_bgzf_inflate(ctx._h, _ptr(image), len(f), _ptr(idx.block_offsets), _ptr(idx.text_offsets), idx.n_blocks, 0, _ptr(got), nt,
                                         _ptr(status), C.byref(bad)))

    def deflate_d2h():
        return buf[:deflate()].cpu()

    def host(level):
        return len(host_compress(d_text.cpu().numpy(), level))

    with torch.cuda.stream(ctx.stream):
        names = ["deflate", "deflate + d2h of the image", "deflate, every block stored", "(a) d2h of the text + host zlib x16, level 1",
                 "(a) d2h of the text + host zlib x16, level 6", "    d2h of the text alone", "(b) copy_ of the text on the device", "inflate of the image (kmx_bgzf_inflate, with CRC)"]
        t = medians([deflate, deflate_d2h, lambda: deflate(_lib.BGZF_DEFLATE_STORED), lambda: host(1), lambda: host(6), lambda: d_text.cpu(),
                     lambda: dst.copy_(d_text), inflate], reps, sync)
    print(f"{'':<58s} {'ms':>9s} {'GB/s':>8s}")
    for name, ms in zip(names, t):
        print(f"{name:<58s} {ms:9.3f} {nt / ms / 1e6:8.2f}")
    print(f"(a) level 1 / (deflate + d2h) = {t[3] / t[1]:.2f}; (a) level 6 / (deflate + d2h) = {t[4] / t[1]:.2f}; the coding kernel = deflate - stored: "
          f"{t[0] - t[2]:.3f} ms; deflate / (b) = {t[0] / t[6]:.1f}; deflate / inflate = {t[0] / t[7]:.2f}")
    held, allocs = ctx.work_buffer_info()
    print(f"work buffer held at the end: {held / 2**20:.1f} MiB ({allocs} allocations)")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
