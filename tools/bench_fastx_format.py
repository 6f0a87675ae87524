"""dev tool: kmx_fastx_format beside a plain copy of as many bytes and beside the cheapest composition outside the new kernel that
yields the same bytes, and kmx_fastx_parse_names beside the read parse of the same image; one process, so that all versions see the
same device state.  The call and the composition are checked equal before anything is timed.
  (a)  Context.fastx_format: the count-only call, the allocation of an exactly sized image, the call that writes it.  Beside it the
       raw call into a buffer that is already there (plan, record offsets and copy) and the count-only call alone (the plan's count
       pass, its scan and the host round trip).  plan = count-only / raw: what of the raw call is not the copy kernel (the offsets
       kernel, a fraction of the count pass, is left with the copy).
  (b)  the composition: the image is a gather of segments.  The constants "@" / ">", "\\n", "\\n+\\n", the names, the bases and the
       quality bytes are concatenated into one source batch (torch.cat) whose reads are the segments; an index of seven (FASTQ) or
       five (FASTA, one line) entries per record names them in output order; kmx_reads_gather copies them.  Timed with the cat
       and the index, as a caller without kmx_fastx_format would run it.  FASTA in lines of 60 has no composition here (the lines
       of a ragged read would have to become source reads of their own): it is set beside the copy only.
  (c)  Tensor.copy_ of as many bytes as (a) writes: the call reads about what it writes, so this is the ceiling.
Two batches: uniform reads of 150 bp, and a ragged mix of 100 .. 160 bp, with the names tests/fastx_cases.fastq_text makes
("@read<i> len=<L>", built on the device).  Three shapes: FASTQ, FASTA in one line, FASTA in lines of 60.  Then the FASTQ image is
parsed: fastx_names (count + emit) beside fastx_parse (count + emit) of the same image.
Times are medians of synchronised runs (ms) between two events on the context's stream, the versions alternating, after three
warm-up calls of each; GB/s = bytes written / time.
Output: profiles/fastx_format_bench.txt.
  python tools/bench_fastx_format.py [n_reads, default 1e7] [reps, default 5]"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

FASTQ, FASTA = 1, 2


def device_names(n, lens, dev):
    """the names of fastq_text on the device: "@read%d len=%d" % (i, L) -> (names uint8, offsets int64[n + 1])"""
    def digits(v, width):
        p = 10 ** torch.arange(width - 1, -1, -1, device=dev, dtype=torch.int64)
        d = (v[:, None] // p[None, :]) % 10 + 48
        live = (v[:, None] >= p[None, :]) | (p[None, :] == 1)
        return d.to(torch.uint8), live

    i_d, i_live = digits(torch.arange(n, device=dev, dtype=torch.int64), 9)
    l_d, l_live = digits(lens, 4)
    head = torch.tensor(list(b"@read"), dtype=torch.uint8, device=dev).expand(n, 5)
    mid = torch.tensor(list(b" len="), dtype=torch.uint8, device=dev).expand(n, 5)
    on = torch.ones(n, 5, dtype=torch.bool, device=dev)
    mat, live = torch.cat([head, i_d, mid, l_d], 1), torch.cat([on, i_live, on, l_live], 1)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(live.sum(1), 0, out=off[1:])
    return mat[live], off


def composition(ctx, fmt, bases, quals, n, read_len, offsets, names, noff):
    """the image as a gather of segments (FASTQ, or FASTA in one line); names from byte 1 on"""
    dev = bases.device
    if offsets is None:
        offsets = torch.arange(n + 1, device=dev, dtype=torch.int64) * read_len
    consts = torch.tensor(list(b"@\n\n+\n" if fmt == FASTQ else b">\n"), dtype=torch.uint8, device=dev)
    c_off = [0, 1, 2] if fmt == FASTQ else [0, 1]        # "@", "\n", "\n+\n" / ">", "\n"
    nc = consts.numel()
    # the source batch: the constants, then for every name its first byte and its rest as two reads, the bases, the quality bytes
    nm = torch.stack([noff[:-1], torch.minimum(noff[:-1] + 1, noff[1:])], 1).reshape(-1)
    parts = [consts, names, bases] + ([quals] if fmt == FASTQ else [])
    offs = [torch.tensor(c_off, device=dev, dtype=torch.int64), nm + nc, offsets[:-1] + (nc + names.numel())]
    if fmt == FASTQ:
        offs.append(offsets[:-1] + (nc + names.numel() + bases.numel()))
    src = torch.cat(parts)
    src_off = torch.cat(offs + [torch.tensor([src.numel()], device=dev, dtype=torch.int64)])
    r = torch.arange(n, device=dev, dtype=torch.int64)
    k = len(c_off)
    name_r, base_r = k + 2 * r + 1, k + 2 * n + r
    # (the last base read would run on into the quality bytes' first: the reads are back to back, so offsets[1:] close them)
    if fmt == FASTQ:
        cols = [torch.zeros_like(r), name_r, torch.ones_like(r), base_r, torch.full_like(r, 2), base_r + n, torch.ones_like(r)]
    else:
        cols = [torch.zeros_like(r), name_r, torch.ones_like(r), base_r, torch.ones_like(r)]
    index = torch.stack(cols, 1).reshape(-1)
    return ctx.reads_gather(src, int(src_off.numel()) - 1, 0, index, offsets=src_off).bases


def median_ms(ctx, fs, reps):
    """medians of `reps` alternating runs of every function of fs between two events, after three warm-up calls of each"""
    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(ctx.stream)
        out = f()
        b.record(ctx.stream)
        torch.cuda.synchronize()
        del out
        return a.elapsed_time(b)

    for f in fs:
        for _ in range(3):
            timed(f)
    t = [[] for _ in fs]
    for _ in range(reps):
        for i, f in enumerate(fs):
            t[i].append(timed(f))
    return [statistics.median(x) for x in t], [(max(x) - min(x)) / statistics.median(x) for x in t]


def race(ctx, name, what, fmt, width, bases, quals, n, read_len, offsets, names, noff, reps, compose):
    from kmers_amd.api import _ptr

    kw = dict(offsets=offsets, quals=quals if fmt == FASTQ else None, names=names, name_offsets=noff, fmt=fmt, line_width=width)
    got = ctx.fastx_format(bases, n, read_len, **kw)
    n_bytes = int(got.numel())
    fs = [lambda: ctx.fastx_format(bases, n, read_len, **kw)]
    if compose:
        want = composition(ctx, fmt, bases, quals, n, read_len, offsets, names, noff)
        if not torch.equal(got, want):
            print(f"{name:<8s} {what:<9s} MISMATCH: the call and its composition differ; not timed")
            return None
        del want
        fs.append(lambda: composition(ctx, fmt, bases, quals, n, read_len, offsets, names, noff))
    r, nm = ctx._reads(bases, n, read_len, offsets), ctx._reads(names, n, 0, noff)
    nb = C.c_uint64(0)
    head = (ctx._h, C.byref(r), _ptr(quals) if fmt == FASTQ else None, C.byref(nm), 1, 0, fmt, width, 73)

    def raw():
        ctx._ck(ctx.lib.kmx_fastx_format(*head, _ptr(got), None, n_bytes, C.byref(nb)))

    def count_only():
        ctx._ck(ctx.lib.kmx_fastx_format(*head, None, None, 0, C.byref(nb)))

    src = torch.empty(n_bytes, dtype=torch.uint8, device=ctx.device)
    dst = torch.empty(n_bytes, dtype=torch.uint8, device=ctx.device)
    with torch.cuda.stream(ctx.stream):
        t, spread = median_ms(ctx, fs + [lambda: dst.copy_(src), raw, count_only], reps)
    a, (c, rw, co) = t[0], t[-3:]
    b = t[1] if compose else float("nan")
    print(f"{name:<8s} {what:<9s} {n_bytes:>10.3e} {a:8.3f} {n_bytes / a / 1e6:8.1f} {rw:8.3f} {n_bytes / rw / 1e6:8.1f} {b:9.3f} {c:8.3f} "
          f"{n_bytes / c / 1e6:8.1f} {b / a:7.2f} {c / a:7.2f} {c / rw:7.2f} {co:8.3f} {co / rw:6.2f} {c / max(rw - co, 1e-9):8.2f} {spread[0]:7.2f}")
    del src, dst
    torch.cuda.empty_cache()
    return got


def main():
    from kmers_amd.api import Context

    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = Context(0)
    dev = ctx.device
    print(f"fastx_format beside a plain copy and the gather composition; {n:.0e} reads; median of {reps} alternating runs each (ms, stream events "
          f"around a synchronise) after 3 warm-up calls; format = Context.fastx_format (count, allocate, write), raw = one kmx_fastx_format call into a "
          f"given buffer; GB/s = bytes written / time; comp = the composition (b: cat, index, kmx_reads_gather; nan: none made); copy = Tensor.copy_ "
          f"of the bytes written (c); b/a = comp / format, c/a = copy / format, c/raw = copy / raw; count = the count-only call; plan = count / raw; "
          f"c/kern = copy / (raw - count): the copy kernel's share of the copy rate; spread = (max - min) / median of format's runs; MI355X")
    print(f"{'batch':<8s} {'shape':<9s} {'bytes out':>10s} {'format':>8s} {'GB/s':>8s} {'raw':>8s} {'GB/s':>8s} {'comp':>9s} {'copy':>8s} {'GB/s':>8s} "
          f"{'b/a':>7s} {'c/a':>7s} {'c/raw':>7s} {'count':>8s} {'plan':>6s} {'c/kern':>8s} {'spread':>7s}")
    g = torch.Generator(device=dev).manual_seed(11)
    images = []
    for name, lo, hi in (("150 bp", 150, 150), ("100-160", 100, 160)):
        if lo == hi:
            lens, offsets, read_len = torch.full((n,), lo, device=dev, dtype=torch.int64), None, lo
        else:
            lens = torch.randint(lo, hi + 1, (n,), device=dev, generator=g)
            offsets = torch.zeros(n + 1, device=dev, dtype=torch.int64)
            torch.cumsum(lens, 0, out=offsets[1:])
            read_len = hi
        total = int(lens.sum())
        bases = ctx.gen_reads(total, seed=0xBEEF)
        quals = (torch.randint(0, 41, (total,), device=dev, generator=g, dtype=torch.int32) + 33).to(torch.uint8)
        names, noff = device_names(n, lens, dev)
        image = race(ctx, name, "FASTQ", FASTQ, 0, bases, quals, n, read_len, offsets, names, noff, reps, True)
        race(ctx, name, "FASTA 0", FASTA, 0, bases, quals, n, read_len, offsets, names, noff, reps, True)
        race(ctx, name, "FASTA 60", FASTA, 60, bases, quals, n, read_len, offsets, names, noff, reps, False)
        images.append((name, image, names, noff))
        del bases, quals, lens, offsets
        torch.cuda.empty_cache()
    print("the names parse of the FASTQ image beside its read parse (count + emit each, the emit reusing the count's summaries)")
    print(f"{'batch':<8s} {'text bytes':>10s} {'names':>8s} {'GB/s':>8s} {'reads':>8s} {'GB/s':>8s} {'names/reads':>11s}")
    for name, image, names, noff in images:
        if image is None:
            continue
        text = torch.empty(image.numel() + 16, dtype=torch.uint8, device=dev)[:image.numel()].copy_(image)       # (16-byte aligned)
        pn, po = ctx.fastx_names(text)
        if not (torch.equal(pn, names) and torch.equal(po, noff)):
            print(f"{name:<8s} MISMATCH: the parsed names are not the names the image was made from; not timed")
            continue
        del pn, po
        with torch.cuda.stream(ctx.stream):
            (tn, tr), _ = median_ms(ctx, [lambda: ctx.fastx_names(text), lambda: ctx.fastx_parse(text, FASTQ)], reps)
        print(f"{name:<8s} {text.numel():>10.3e} {tn:8.3f} {text.numel() / tn / 1e6:8.1f} {tr:8.3f} {text.numel() / tr / 1e6:8.1f} {tn / tr:11.2f}")
    held, allocs = ctx.work_buffer_info()
    print(f"work buffer held at the end: {held / 2**30:.2f} GiB ({allocs} allocations)")
    ctx.close()


if __name__ == "__main__":
    main()
