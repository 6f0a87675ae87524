"""dev tool: kmx_bgzf_index and kmx_bgzf_inflate beside the host path they replace and beside a plain copy; one process, so that all
versions see the same device state.  The inflated text is checked equal to the host's before anything is timed.
  input  a FASTQ image of n reads of 150 bp (tests/fastx_cases.fastq_text names and alphabets, made in pieces), compressed with
         bgzf_compress at level 6 by a thread pool of at most 16 (zlib releases the GIL).
  index      kmx_bgzf_index into arrays that are there (candidates, chain marking, ranks, ISIZE scan; four host round trips)
  inflate    kmx_bgzf_inflate with the CRC-32 kernel, and with KMX_BGZF_NO_CRC: the difference is the CRC kernel
  ingest     Context.load_fastx (copy of the compressed bytes, index, inflate) + fastq_records: a file's bytes to reads, qualities, names
  (a) host   zlib.decompress of the same blocks over 16 threads, plus the host-to-device copy of the text: what a caller does today
  h2d        the host-to-device copy of the compressed bytes (pageable memory, as load_fastx makes it): inflate + h2d is what is set
             beside (a)
  (b) copy   Tensor.copy_ of the text's bytes on the device: the ceiling of anything that writes the text
Times are medians of synchronised runs (ms, wall clock between two synchronises: most of what is timed involves the host),
the versions alternating, after two warm-up calls of each; GB/s = bytes of text / time.
Output: profiles/bgzf_bench.txt.
  python tools/bench_bgzf.py [n_reads, default 2e6] [reps, default 5]"""
import ctypes as C
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

THREADS = min(16, os.cpu_count() or 1)


def make_text(n):
    """what tests/fastx_cases.fastq_text(fixed=150) writes, with the bases and quality bytes drawn a matrix at a time"""
    from tests.fastx_cases import QUAL_ALPHA, SEQ_ALPHA

    def piece(i):
        rng, m, first = np.random.default_rng(1000 + i), min(20000, n - i * 20000), i * 20000
        rows = []
        for alpha in (SEQ_ALPHA, QUAL_ALPHA):
            a = np.empty((m, 151), np.uint8)
            a[:, :150] = rng.choice(np.asarray(alpha, np.uint8), (m, 150))
            a[:, 150] = 10
            rows.append(a.tobytes())
        s, q = rows
        return b"".join(b"@read%d len=150\n%s+\n%s" % (first + r, s[151 * r:151 * r + 151], q[151 * r:151 * r + 151]) for r in range(m))

    with ThreadPoolExecutor(THREADS) as ex:
        return b"".join(ex.map(piece, range((n + 19999) // 20000)))


def compress(text):
    from kmers_amd.api import BGZF_EOF, bgzf_compress

    step = 65280 * 64
    with ThreadPoolExecutor(THREADS) as ex:
        parts = list(ex.map(lambda i: bgzf_compress(memoryview(text)[i:i + step], 6)[:-28], range(0, len(text), step)))
    return b"".join(parts) + BGZF_EOF


def host_inflate(f, bo):
    def one(b):
        return zlib.decompress(memoryview(f)[bo[b] + 18:bo[b + 1] - 8], -15)

    with ThreadPoolExecutor(THREADS) as ex:
        return b"".join(ex.map(one, range(len(bo) - 1), chunksize=64))


def medians(fs, reps, sync):
    def timed(f):
        sync()
        t0 = time.perf_counter()
        out = f()
        sync()
        dt = (time.perf_counter() - t0) * 1e3
        del out
        return dt

    for f in fs:
        for _ in range(2):
            timed(f)
    t = [[] for _ in fs]
    for _ in range(reps):
        for i, f in enumerate(fs):
            t[i].append(timed(f))
    return [statistics.median(x) for x in t]


def main():
    from kmers_amd import _lib
    from kmers_amd.api import Context, _ptr

    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 2_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    t0 = time.perf_counter()
    text = make_text(n)
    f = compress(text)
    print(f"bgzf: {n:.0e} FASTQ reads of 150 bp, {len(text):.3e} bytes of text, {len(f):.3e} compressed (level 6, ratio {len(text) / len(f):.2f}); "
          f"built in {time.perf_counter() - t0:.1f} s by {THREADS} threads; median of {reps} alternating runs each (ms) after 2 warm-up calls; "
          f"GB/s = bytes of text / time; MI355X")
    ctx = Context(0)
    sync = torch.cuda.synchronize
    image = ctx.to_device(f)
    idx = ctx.bgzf_index(image)
    got = ctx.bgzf_inflate(image, idx)
    if got.cpu().numpy().tobytes() != text:
        print("MISMATCH: the inflated text is not the host's; not timed")
        return 1
    bo = [int(x) for x in idx.block_offsets.cpu().numpy()]
    if host_inflate(f, bo) != text:
        print("MISMATCH: the host path does not give the text back; not timed")
        return 1
    nb, nt = idx.n_blocks, idx.n_text_bytes
    print(f"{nb} blocks; the inflated text equals the host's, byte for byte")
    info = (C.c_uint64 * 4)()
    bad = C.c_uint64(0)
    status = torch.zeros(nb, dtype=torch.int32, device=ctx.device)
    dst = torch.empty(nt, dtype=torch.uint8, device=ctx.device)

    def index():
        ctx._ck(ctx.lib.kmx_bgzf_index(ctx._h, _ptr(image), len(f), _ptr(idx.block_offsets), _ptr(idx.text_offsets), nb, info))

    def inflate(flags):
        ctx._ck(ctx.lib.kmx_bgzf_inflate(ctx._h, _ptr(image), len(f), _ptr(idx.block_offsets), _ptr(idx.text_offsets), nb, flags, _ptr(got), nt,
                                         _ptr(status), C.byref(bad)))

    def host():
        return torch.from_numpy(np.frombuffer(host_inflate(f, bo), np.uint8)).to(ctx.device)

    def host_only():
        return len(host_inflate(f, bo))

    with torch.cuda.stream(ctx.stream):
        names = ["index", "inflate", "inflate, no CRC", "ingest (load_fastx + fastq_records)", "(a) host zlib x16 + copy of the text", "    host zlib x16 alone",
                 "h2d of the compressed bytes", "(b) copy_ of the text on the device"]
        t = medians([index, lambda: inflate(0), lambda: inflate(_lib.BGZF_NO_CRC), lambda: ctx.fastq_records(ctx.load_fastx(f)), host, host_only,
                     lambda: ctx.to_device(f), lambda: dst.copy_(got)], reps, sync)
    print(f"{'':<40s} {'ms':>9s} {'GB/s':>8s}")
    for name, ms in zip(names, t):
        print(f"{name:<40s} {ms:9.3f} {nt / ms / 1e6:8.2f}")
    dev_path, host_path = t[0] + t[1] + t[6], t[4]
    print(f"index + inflate + h2d of the compressed bytes: {dev_path:.3f} ms; (a): {host_path:.3f} ms; (a) / device path = {host_path / dev_path:.2f}")
    print(f"CRC kernel = inflate - inflate without: {t[1] - t[2]:.3f} ms; inflate / (b) = {t[1] / t[7]:.1f}")
    held, allocs = ctx.work_buffer_info()
    print(f"work buffer held at the end: {held / 2**20:.1f} MiB ({allocs} allocations)")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
