"""dev tool: the counting sketch beside the calls it stands next to, on one batch in one process.
  (a)  add:    Context.sketch_add(2): the windows call into the work buffer, then the add kernel (four compare-and-swaps a window,
               fewer where a cell is saturated).
  (b)  lookup: Context.sketch_lookup_reads(2): the windows call, then four byte loads of one line per window.
  (c)  min:    Context.count_canonical_min(2) at min_est = 2 against the sketch of (a): the exact counter over what the sketch lets through.
       each at log2_blocks = 20, 26 and 30 (64 MiB, 4 GiB, 64 GiB of cells), and beside them, once:
  (d)  hist:   kmx_histogram (lex hash) of the same batch at 2^26 buckets (u64 counters; the partitioned passes) -- one-word k only.
  (e)  count:  Context.count_canonical(2), unfiltered.
  (f)  copy:   Tensor.copy_ of as many bytes as the windows call writes (9 or 17 per window).
Then count_solid(2) over the batch cut into four against count-each + count_merge + count_filter, with the largest table either holds
on the way.  The reads are drawn from one random genome (30x coverage at the defaults) with 1 % substitutions, forward strand: most
distinct k-mers are errors that occur once, the case the sketch is for; random reads would make every k-mer a singleton.
Times are wall-clock medians of synchronised calls (ms) after one warm-up call of each, the contestants alternating.
Output: profiles/sketch_bench.txt.
  python tools/bench_sketch.py [n_reads, default 1e7] [reps, default 3] [k ..., default 31 47]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from tools.bench_reads_adapter import timed

L = 150
SUB = 0.01
LOG2 = (20, 26, 30)


def make_reads(ctx, n, g):
    """-> uint8[n * L]: reads of L bases from a genome of n * L / 30 bases, each base substituted with probability SUB"""
    dev = ctx.device
    genome = ctx.gen_reads(max(n * L // 30, 4 * L), seed=0x5CE7C4)
    out = torch.empty(n * L, dtype=torch.uint8, device=dev)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    code = torch.zeros(256, dtype=torch.int64, device=dev)
    code[list(b"ACGT")] = torch.arange(4, device=dev)
    ar = torch.arange(L, device=dev)
    for a in range(0, n, 1 << 20):   # (a chunk of reads at a time: the gather's indices are eight times the chunk)
        m = min(1 << 20, n - a)
        starts = torch.randint(0, genome.numel() - L, (m,), device=dev, generator=g)
        piece = genome[starts[:, None] + ar]
        hit = torch.rand(m, L, device=dev, generator=g) < SUB
        other = acgt[(code[piece.long()] + torch.randint(1, 4, (m, L), device=dev, generator=g)) % 4]
        out[a * L:(a + m) * L] = torch.where(hit, other, piece).reshape(-1)
    return out


def medians(fs, reps):
    for f in fs:
        _, o = timed(f)
        del o
    t = [[] for _ in fs]
    for _ in range(reps):
        for i, f in enumerate(fs):
            ms, o = timed(f)
            t[i].append(ms)
            del o
    return [statistics.median(x) for x in t]


def calls_of(ctx, k):
    if k <= 31:
        return ctx.sketch_add, ctx.sketch_lookup_reads, ctx.count_canonical_min, ctx.count_canonical, ctx.count_merge, ctx.count_filter, ctx.count_solid
    return ctx.sketch_add2, ctx.sketch_lookup_reads2, ctx.count_canonical_min2, ctx.count_canonical2, ctx.count_merge2, ctx.count_filter2, ctx.count_solid2


def bench_k(ctx, bases, n, k, reps):
    from kmers_amd._lib import HASH_LEX

    add, lookup, cmin, count, merge, flt, solid = calls_of(ctx, k)
    win = n * (L - k + 1)
    per = 9 if k <= 31 else 17
    src = torch.empty(win * per, dtype=torch.uint8, device=ctx.device)
    dst = torch.empty_like(src)
    est = torch.empty(win, dtype=torch.uint8, device=ctx.device)
    fs = [lambda: count(bases, n, L, k)[1].numel(), lambda: dst.copy_(src)]
    names = ["count", "copy"]
    if k <= 31:
        hist = torch.zeros(1 << 26, dtype=torch.int64, device=ctx.device)
        fs.append(lambda: ctx.histogram(bases, n, L, k, HASH_LEX, k, 26, counts=hist))
        names.append("hist 2^26")
    with torch.cuda.stream(ctx.stream):
        base = medians(fs, reps)
    n_full = count(bases, n, L, k)[1].numel()
    for nm, ms in zip(names, base):
        print(f"k={k:<3d} {nm:<12s} {'-':>5s} {ms:10.2f} ms {win / ms / 1e6:9.2f} Gwin/s", flush=True)
    print(f"k={k:<3d} {'':<12s} windows {win:.3e}, distinct k-mers {n_full:.3e}", flush=True)
    del src, dst
    torch.cuda.empty_cache()
    for lb in LOG2:
        try:
            s = add(ctx.sketch_new(lb), bases, n, L, k)
        except (RuntimeError, torch.cuda.OutOfMemoryError) as exc:   # noqa: PERF203  (a sketch the device has no room for)
            print(f"k={k:<3d} log2_blocks {lb}: not run ({type(exc).__name__})", flush=True)
            continue
        fill = s.fill()
        n_min = cmin(s, 2, bases, n, L, k, count_only=True)
        scratch = ctx.sketch_new(lb)
        with torch.cuda.stream(ctx.stream):
            a, b, c = medians([lambda: add(scratch, bases, n, L, k), lambda: lookup(s, bases, n, L, k, out=est),
                               lambda: cmin(s, 2, bases, n, L, k)[1].numel()], reps)
        for nm, ms in (("add", a), ("lookup", b), ("min (est>=2)", c)):
            print(f"k={k:<3d} {nm:<12s} {lb:>5d} {ms:10.2f} ms {win / ms / 1e6:9.2f} Gwin/s", flush=True)
        print(f"k={k:<3d} {'':<12s} {lb:>5d} fill {fill:.4f}, table at min_est = 2: {n_min:.3e} of {n_full:.3e} distinct k-mers", flush=True)
        del s, scratch
        torch.cuda.empty_cache()
    # four batches: the two-pass count beside count-each + merge + filter
    q = n // 4
    batches = [(bases[i * q * L:(i + 1) * q * L], q, L, None) for i in range(4)]

    def each():
        km, ct, top = None, None, 0
        for b, nb, rl, off in batches:
            bk, bc = count(b, nb, rl, k, offsets=off)
            km, ct = (bk, bc) if km is None else merge(km, ct, bk, bc)
            top = max(top, int(bc.numel()), int(ct.numel()))
        km, ct = flt(km, ct, 2, 2**64 - 1)
        return int(ct.numel()), top

    def two_pass(lb):
        sizes = []
        km, ct, _ = solid(batches, k, 2, lb, tables=sizes)
        return int(ct.numel()), max(sizes)

    lb = 26
    with torch.cuda.stream(ctx.stream):
        (n_a, top_a), (n_b, top_b) = each(), two_pass(lb)
        a, b = medians([each, lambda: two_pass(lb)], reps)
    print(f"k={k:<3d} four batches of {q:.2e} reads: count-each + merge + filter {a:10.2f} ms, largest table {top_a:.3e}; "
          f"count_solid(log2_blocks = {lb}) {b:10.2f} ms, largest batch table {top_b:.3e}; solid k-mers {n_a:.3e} / {n_b:.3e} "
          f"({'equal' if n_a == n_b else 'DIFFERENT'})", flush=True)


def main():
    from kmers_amd.api import Context

    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    ks = [int(a) for a in sys.argv[3:]] or [31, 47]
    ctx = Context(0)
    ctx.set_work_buffer_limit(48 << 30)   # (the two-word counter's 36 bytes a window at 1e7 reads are above the automatic cap)
    print(f"the counting sketch beside kmx_histogram, the unfiltered counter and a plain copy; {n:.0e} uniform reads of {L} bp from a genome at 30x "
          f"with {SUB:.0%} substitutions; work buffer cap 48 GiB; median of {reps} alternating wall-clock runs each (ms) after 1 warm-up call; "
          f"Gwin/s = windows / time; add = sketch_add, lookup = sketch_lookup_reads, min = count_canonical_min(min_est = 2), count = count_canonical, "
          f"copy = Tensor.copy_ moving the bytes the windows call writes; MI355X", flush=True)
    g = torch.Generator(device=ctx.device).manual_seed(21)
    bases = make_reads(ctx, n, g)
    for k in ks:
        bench_k(ctx, bases, n, k, reps)
    ctx.close()


if __name__ == "__main__":
    main()
