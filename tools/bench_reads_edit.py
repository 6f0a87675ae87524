"""dev tool: kmx_reads_select beside the torch composition that produces the same bytes and beside a plain copy of as many bytes, in
one process so that all three see the same device state; the call and the composition are checked equal before anything is timed.
  (a)  Context.reads_select: the count-only call, the allocation of exactly sized outputs, the call that writes them.  Beside it the
       raw call into buffers that are already there (one call: plan and copy), the count-only call alone (the plan's count pass, its
       scan and the host round trip) and the plan's write pass, measured as the raw call less the count-only call on the same batch
       with every clip empty -- as many output reads, no byte to copy.  plan = count-only + write pass; its share is of the raw call.
  (b)  torch on the device: clip starts and lengths from the keep bytes and span words, cumsum -> output offsets, repeat_interleave of
       the output read per byte, arange less the read's output offset plus its source start -> the source position of every byte, a
       byte gather.
  (c)  Tensor.copy_ of as many bytes as (a) writes: one byte read and one written per kept base, the ceiling.
Two batches: uniform reads of 150 bp, and a ragged mix of 100 .. 160 bp.  Two selections each: half of the reads kept whole (random
keep bytes), and every read kept and trimmed to a span of windows (span_k = 31; the span words lie in column RS_SPAN of an
[n_reads, 8] tensor of rows, as count_read_stats leaves them, and are read in place: stride 8).  The span words are drawn, not
computed from a table: start in 0 .. 39, 31 windows or more, up to the read's end.  Times are wall-clock medians of synchronised calls (ms) after three
warm-up calls of each; GB/s = bytes written / time.
Output: profiles/reads_edit_bench.txt.
  python tools/bench_reads_edit.py [n_reads, default 1e7] [reps, default 5]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

K = 31


def composition(bases, n_reads, read_len, offsets, keep, span, span_k):
    """-> (out bases, out offsets int64[n_out + 1]) for well-formed spans (start < 2^31, no wrap): the rule of include/kmx.h in torch"""
    dev = bases.device
    if offsets is None:
        a = torch.arange(n_reads, device=dev, dtype=torch.int64) * read_len
        length = torch.full((n_reads,), read_len, device=dev, dtype=torch.int64)
    else:
        a, length = offsets[:-1], offsets[1:] - offsets[:-1]
    start = torch.zeros_like(a)
    if span is not None:
        start, ln = span & 0xFFFFFFFF, (span >> 32) & 0xFFFFFFFF
        if span_k:
            ln = torch.where(ln > 0, ln + (span_k - 1), ln)
        inside = start < length
        start = torch.where(inside, start, torch.zeros_like(start))
        length = torch.where(inside, torch.minimum(ln, length - start), torch.zeros_like(ln))
    if keep is not None:
        kept = keep != 0
        a, start, length = a[kept], start[kept], length[kept]
    out_off = torch.zeros(length.numel() + 1, device=dev, dtype=torch.int64)
    torch.cumsum(length, 0, out=out_off[1:])
    total = int(out_off[-1])
    read = torch.repeat_interleave(torch.arange(length.numel(), device=dev), length, output_size=total)
    pos = torch.arange(total, device=dev, dtype=torch.int64) - out_off[read] + (a + start)[read]
    return bases[pos], out_off


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median_ms(fs, reps):
    """medians of `reps` alternating runs of every function of fs, after three warm-up calls of each"""
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


def race(ctx, name, what, bases, n, read_len, offsets, keep, span, span_k, reps):
    from kmers_amd.api import _ptr

    args = dict(keep=keep, span=span, span_k=span_k, offsets=offsets)
    _, got = timed(lambda: ctx.reads_select(bases, n, read_len, **args))
    _, want = timed(lambda: composition(bases, n, read_len, offsets, keep, span, span_k))
    if not (torch.equal(got.bases, want[0]) and torch.equal(got.offsets, want[1])):
        print(f"{name:<8s} {what:<10s} MISMATCH: the call and its composition differ; not timed")
        return
    n_out, n_bases = got.n_reads, got.n_bases
    del want
    # the raw call into buffers that are there, the count-only call, and the write pass alone (every clip empty: no byte to copy)
    r = ctx._reads(bases, n, read_len, offsets)
    span_t, span_p, stride = ctx._span_arg(span)
    empty = torch.zeros(n, dtype=torch.int64, device=ctx.device)
    off2 = torch.empty(n + 1, dtype=torch.int64, device=ctx.device)
    nr, nb = C.c_uint64(0), C.c_uint64(0)
    head = (ctx._h, C.byref(r), _ptr(keep), span_p, stride, span_k, 0)
    head0 = (ctx._h, C.byref(r), _ptr(keep), _ptr(empty), 1, 0, 0)

    def raw():
        ctx._ck(ctx.lib.kmx_reads_select(*head, _ptr(got.bases), _ptr(got.offsets), None, n_out, n_bases, C.byref(nr), C.byref(nb)))

    def count_only():
        ctx._ck(ctx.lib.kmx_reads_select(*head, None, None, None, 0, 0, C.byref(nr), C.byref(nb)))

    def write_only():
        ctx._ck(ctx.lib.kmx_reads_select(*head0, _ptr(got.bases), _ptr(off2), None, n, max(n_bases, 1), C.byref(nr), C.byref(nb)))

    def count_only0():
        ctx._ck(ctx.lib.kmx_reads_select(*head0, None, None, None, 0, 0, C.byref(nr), C.byref(nb)))

    src = torch.empty(n_bases, dtype=torch.uint8, device=ctx.device)
    dst = torch.empty(n_bases, dtype=torch.uint8, device=ctx.device)
    with torch.cuda.stream(ctx.stream):
        (a, b, c, rw, co, w0, c0), spread = median_ms([lambda: ctx.reads_select(bases, n, read_len, **args),
                                                        lambda: composition(bases, n, read_len, offsets, keep, span, span_k),
                                                        lambda: dst.copy_(src), raw, count_only, write_only, count_only0], reps)
    plan = co + max(w0 - c0, 0.0)
    print(f"{name:<8s} {what:<10s} {n_out:>10.3e} {n_bases:>10.3e} {a:8.3f} {n_bases / a / 1e6:8.1f} {rw:8.3f} {n_bases / rw / 1e6:8.1f} {b:9.3f} "
          f"{c:8.3f} {n_bases / c / 1e6:8.1f} {b / a:7.2f} {c / a:7.2f} {c / rw:7.2f} {co:8.3f} {max(w0 - c0, 0.0):8.3f} {plan / rw:6.2f} {spread[0]:7.2f}")
    del got, src, dst
    torch.cuda.empty_cache()


def main():
    from kmers_amd._lib import RS_SPAN, RS_WORDS
    from kmers_amd.api import Context

    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = Context(0)
    dev = ctx.device
    print(f"reads_select beside its torch composition and a plain copy; {n:.0e} reads; median of {reps} alternating wall-clock runs each (ms) "
          f"after 3 warm-up calls; select = Context.reads_select (count, allocate, write), raw = one kmx_reads_select call into given buffers; "
          f"GB/s = bytes written / time; comp = the torch composition (b); copy = Tensor.copy_ of the bytes written (c); b/a = comp / select, "
          f"c/a = copy / select, c/raw = copy / raw; count = the count-only call; write = the plan's write pass; plan = (count + write) / raw; "
          f"spread = (max - min) / median of select's runs; MI355X")
    print(f"{'batch':<8s} {'selection':<10s} {'reads out':>10s} {'bytes out':>10s} {'select':>8s} {'GB/s':>8s} {'raw':>8s} {'GB/s':>8s} {'comp':>9s} "
          f"{'copy':>8s} {'GB/s':>8s} {'b/a':>7s} {'c/a':>7s} {'c/raw':>7s} {'count':>8s} {'write':>8s} {'plan':>6s} {'spread':>7s}")
    g = torch.Generator(device=dev).manual_seed(11)
    keep = (torch.rand(n, device=dev, generator=g) < 0.5).to(torch.uint8)
    for name, lo, hi in (("150 bp", 150, 150), ("100-160", 100, 160)):
        if lo == hi:
            lens, offsets, read_len = torch.full((n,), lo, device=dev, dtype=torch.int64), None, lo
        else:
            lens = torch.randint(lo, hi + 1, (n,), device=dev, generator=g)
            offsets = torch.zeros(n + 1, device=dev, dtype=torch.int64)
            torch.cumsum(lens, 0, out=offsets[1:])
            read_len = hi
        bases = ctx.gen_reads(int(lens.sum()), seed=0xBEEF)
        rows = torch.zeros(n, RS_WORDS, device=dev, dtype=torch.int64)
        start = torch.randint(0, 40, (n,), device=dev, generator=g)
        most = lens - (K - 1) - start                          # the windows from `start` to the read's end: at least 31
        wins = 31 + (torch.rand(n, device=dev, generator=g, dtype=torch.float64) * (most - 30)).to(torch.int64)
        rows[:, RS_SPAN] = start | (wins << 32)
        del start, most, wins
        race(ctx, name, "half kept", bases, n, read_len, offsets, keep, None, 0, reps)
        race(ctx, name, "trimmed", bases, n, read_len, offsets, None, rows[:, RS_SPAN], K, reps)
        del bases, rows, lens, offsets
        torch.cuda.empty_cache()
    held, allocs = ctx.work_buffer_info()
    print(f"work buffer held at the end: {held / 2**30:.2f} GiB ({allocs} allocations)")
    ctx.close()


if __name__ == "__main__":
    main()
