"""dev tool: kmx_reads_quality beside the torch composition that produces the same masked bytes and the same LOW / QSUM / RUN words, and
beside a plain copy of the bytes the call moves; then kmx_fastx_parse_quals beside kmx_fastx_parse on one FASTQ image.  One process,
so that everything sees the same device state; the call and the composition are checked equal before anything is timed.
  (a)  kmx_reads_quality into buffers that are there: the masked copy and the rows (min_q = 20, trim_q = 20, k = 31, the "ee" weight
       table), and the rows alone (no masked copy).
  (b)  torch on the device: q from the quality bytes, the masked bytes by a where, LOW and QSUM by segment sums, the longest run of good
       bases by a cummax of "last position that is not good" over the flat batch (a read's start counts as one), a packed
       (length, leftmost) key and a segment maximum.
  (c)  Tensor.copy_ of 3 bytes per base: two read and one written per base is what (a) moves; the ceiling.
Two batches: uniform reads of 150 bp and a ragged mix of 100 .. 160 bp; quality bytes drawn from a two-level mix (90 % Q30..Q40,
10 % Q2..Q19) so that masked bases, runs and trim spans all occur.
  (d)  the quality parse: Context.fastx_quals beside Context.fastx_parse (counts + emit each) on an image of 150-bp records, and
       fastx_quals with same_text=True right behind a fastx_parse (pass 1 not repeated).
Times are wall-clock medians of synchronised calls (ms) after three warm-up calls of each, the contestants alternating.
Output: profiles/reads_quality_bench.txt.
  python tools/bench_reads_quality.py [n_reads, default 1e7] [reps, default 5]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

MIN_Q, TRIM_Q, K, PHRED = 20, 20, 31, 33


def composition(bases, quals, n, offsets):
    """-> (masked, low int64[n], qsum int64[n], run word int64[n]); offsets int64[n + 1] (uniform reads: an arange)"""
    dev = bases.device
    total = bases.numel()
    lens = offsets[1:] - offsets[:-1]
    q = (quals.to(torch.int16) - PHRED).clamp_(min=0)
    low = q < MIN_Q
    masked = torch.where(low, torch.full_like(bases, ord("N")), bases)
    read = torch.repeat_interleave(torch.arange(n, device=dev), lens, output_size=total)
    n_low = torch.zeros(n, device=dev, dtype=torch.int64).scatter_add_(0, read, low.to(torch.int64))
    qsum = torch.zeros(n, device=dev, dtype=torch.int64).scatter_add_(0, read, q.to(torch.int64))
    u = bases & 0xDF
    good = ((u == ord("A")) | (u == ord("C")) | (u == ord("G")) | (u == ord("T"))) & ~low
    del q, low, u
    pos = torch.arange(total, device=dev, dtype=torch.int64)
    start = offsets[:-1][read]
    last_bad = torch.cummax(torch.where(good, start, pos + 1), 0).values
    run = pos + 1 - last_bad                                     # the run of good bases that ends here
    key = (run << 32) | (0xFFFFFFFF - (pos + 1 - run - start))   # longest, then leftmost
    del pos, last_bad, good
    best = torch.zeros(n, device=dev, dtype=torch.int64).scatter_reduce_(0, read, key, "amax", include_self=True)
    ln = best >> 32
    word = torch.where(ln > 0, (0xFFFFFFFF - (best & 0xFFFFFFFF)) | (ln << 32), torch.zeros_like(ln))
    return masked, n_low, qsum, word


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median_ms(fs, reps):
    for f in fs:
        for _ in range(3):
            _, o = timed(f)
            del o
    t = [[] for _ in fs]
    for _ in range(reps):
        for i, f in enumerate(fs):
            ms, o = timed(f)
            t[i].append(ms)
            del o
    return [statistics.median(x) for x in t], [(max(x) - min(x)) / statistics.median(x) for x in t]


def race(ctx, name, bases, quals, n, read_len, offsets, reps):
    from kmers_amd import _lib
    from kmers_amd.api import _ptr, ee_weights

    dev = ctx.device
    flat = offsets if offsets is not None else torch.arange(n + 1, device=dev, dtype=torch.int64) * read_len
    w = ctx.to_device(ee_weights(PHRED))
    masked = torch.empty_like(bases)
    rows = torch.empty(n * _lib.RQ_WORDS, dtype=torch.int64, device=dev)
    r = ctx._reads(bases, n, read_len, offsets)

    def call(m):
        ctx._ck(ctx.lib.kmx_reads_quality(ctx._h, C.byref(r), _ptr(quals), PHRED, MIN_Q, TRIM_Q, K, _ptr(w), _ptr(m) if m is not None else None, _ptr(rows)))

    timed(lambda: call(masked))
    _, want = timed(lambda: composition(bases, quals, n, flat))
    rw = rows.view(n, _lib.RQ_WORDS)
    same = (torch.equal(masked, want[0]) and torch.equal(rw[:, _lib.RQ_LOW], want[1]) and torch.equal(rw[:, _lib.RQ_QSUM], want[2])
            and torch.equal(rw[:, _lib.RQ_RUN], want[3]))
    n_masked = int(want[1].sum())
    del want
    torch.cuda.empty_cache()
    if not same:
        print(f"{name:<8s} MISMATCH: the call and its composition differ; not timed")
        return
    nb = bases.numel()
    half = (3 * nb) // 2                                          # copy_ of 1.5 bytes per base reads 1.5 and writes 1.5: 3 moved
    src = torch.empty(half, dtype=torch.uint8, device=dev)
    dst = torch.empty(half, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(ctx.stream):
        (a, a0, b, c), spread = median_ms([lambda: call(masked), lambda: call(None), lambda: composition(bases, quals, n, flat),
                                          lambda: dst.copy_(src)], reps)
    moved = 3 * nb + 64 * n
    print(f"{name:<8s} {n:>10.3e} {nb:>10.3e} {n_masked / nb:7.3f} {a:8.3f} {moved / a / 1e6:8.1f} {a0:8.3f} {b:9.3f} {c:8.3f} {3 * nb / c / 1e6:8.1f} "
          f"{b / a:7.2f} {c / a:7.2f} {spread[0]:7.2f}")
    del src, dst, masked, rows
    torch.cuda.empty_cache()


def parse_race(ctx, reps):
    rng = np.random.default_rng(7)
    recs = []
    for i in range(65536):
        seq = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=150))
        qual = bytes(rng.integers(33 + 2, 33 + 41, 150).astype(np.uint8))
        recs.append(b"@SRR000000.%d %d/1\n" % (i, i) + seq + b"\n+\n" + qual + b"\n")
    text = ctx.to_device(np.frombuffer(b"".join(recs), dtype=np.uint8).copy()).repeat(64)
    bases, offsets = ctx.fastx_parse(text, 1)
    quals, qoffsets = ctx.fastx_quals(text, offsets)
    assert torch.equal(offsets, qoffsets)
    del bases, quals

    def both():
        b, o = ctx.fastx_parse(text, 1)
        return ctx.fastx_quals(text, o, same_text=True)

    with torch.cuda.stream(ctx.stream):
        (p, q, pq), spread = median_ms([lambda: ctx.fastx_parse(text, 1), lambda: ctx.fastx_quals(text), both], reps)
    gb = text.numel() / 1e6
    print(f"quality parse: {text.numel() / 1e9:.2f} GB of text, {offsets.numel() - 1} records: fastx_parse {p:.3f} ms ({gb / p:.0f} GB/s of text), "
          f"fastx_quals {q:.3f} ms ({gb / q:.0f} GB/s), fastx_parse then fastx_quals(same_text, with the length check) {pq:.3f} ms "
          f"(the two apart: {p + q:.3f}); quals / parse = {q / p:.2f}; spread of fastx_quals {spread[1]:.2f}")


def main():
    from kmers_amd.api import Context

    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = Context(0)
    dev = ctx.device
    print(f"reads_quality beside its torch composition and a plain copy; {n:.0e} reads; min_q = {MIN_Q}, trim_q = {TRIM_Q}, k = {K}, weights \"ee\"; "
          f"median of {reps} alternating wall-clock runs each (ms) after 3 warm-up calls; call = kmx_reads_quality (masked copy + rows) into given "
          f"buffers, GB/s = (3 bytes per base + 64 per read) / time; rows = the same call without the masked copy; comp = the torch composition "
          f"(masked bytes, LOW, QSUM, RUN); copy = Tensor.copy_ moving 3 bytes per base, GB/s = bytes moved / time; b/a = comp / call, "
          f"c/a = copy / call; masked = share of the bases below min_q; spread = (max - min) / median of the call's runs; MI355X")
    print(f"{'batch':<8s} {'reads':>10s} {'bases':>10s} {'masked':>7s} {'call':>8s} {'GB/s':>8s} {'rows':>8s} {'comp':>9s} {'copy':>8s} {'GB/s':>8s} "
          f"{'b/a':>7s} {'c/a':>7s} {'spread':>7s}")
    g = torch.Generator(device=dev).manual_seed(11)
    for name, lo, hi in (("150 bp", 150, 150), ("100-160", 100, 160)):
        if lo == hi:
            total, offsets, read_len = n * lo, None, lo
        else:
            lens = torch.randint(lo, hi + 1, (n,), device=dev, generator=g)
            offsets = torch.zeros(n + 1, device=dev, dtype=torch.int64)
            torch.cumsum(lens, 0, out=offsets[1:])
            total, read_len = int(offsets[-1]), hi
        bases = ctx.gen_reads(total, seed=0xBEEF)
        hi_q = torch.randint(PHRED + 30, PHRED + 41, (total,), device=dev, generator=g, dtype=torch.uint8)
        lo_q = torch.randint(PHRED + 2, PHRED + 20, (total,), device=dev, generator=g, dtype=torch.uint8)
        quals = torch.where(torch.rand(total, device=dev, generator=g) < 0.9, hi_q, lo_q)
        del hi_q, lo_q
        race(ctx, name, bases, quals, n, read_len, offsets, reps)
        del bases, quals, offsets
        torch.cuda.empty_cache()
    parse_race(ctx, reps)
    ctx.close()


if __name__ == "__main__":
    main()
