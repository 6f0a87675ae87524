"""dev tool: the distinct-key estimator beside the counting sketch, on the batch of tools/bench_sketch.py in one process.
  (a)  words:  Context.hll_add_words over the canon array of canonical_windows (8 bytes read per key, one register read, an atomic
               only where the rank is larger) beside Context.sketch_add_words over the same array (four compare-and-swaps a key)
               and a plain Tensor.copy_ of the 8 bytes per key both read.
  (b)  reads:  Context.hll_add beside Context.sketch_add: the windows call into the work buffer, then the add kernel.
  (c)  routes: hll_add_words at log2_regs 9 / 14 (block-private LDS registers) and 15 / 18 / 24 (global compare-and-swap) over all
               keys, and at 14 over a head of the array one key short of the keys-per-block cut (global) and at the cut (block-private).
  (d)  the estimate beside count_canonical's n_distinct, and the sketch it sizes.
Reads: bench_sketch.make_reads (uniform 150 bp from a genome at 30x with 1% substitutions).

Output: profiles/hll_bench.txt.
  python tools/bench_hll.py [n_reads ..., default 2e5 1e7] [--reps R, default 3] [--k K, default 31]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from tools.bench_sketch import L, make_reads, medians


def bench(ctx, n, k, reps):
    from kmers_amd import _lib

    two = k > 31
    windows, hll_add, hll_words, sk_add, sk_words, count = (
        (ctx.canonical_windows2, ctx.hll_add2, ctx.hll_add_words2, ctx.sketch_add2, ctx.sketch_add_words2, ctx.count_canonical2) if two else
        (ctx.canonical_windows, ctx.hll_add, ctx.hll_add_words, ctx.sketch_add, ctx.sketch_add_words, ctx.count_canonical))
    g = torch.Generator(device=ctx.device).manual_seed(21)
    bases = make_reads(ctx, n, g)
    win = n * (L - k + 1)
    n_distinct = int(count(bases, n, L, k)[1].numel())
    torch.cuda.empty_cache()
    canon = windows(bases, n, L, k) if two else windows(bases, n, L, k, want=("canon", "flags"))
    canon = canon["canon"]                                    # (every window of these reads is valid: ACGT only)
    words = 2 if two else 1
    src = canon.view(-1)
    dst = torch.empty_like(src)
    p0 = 14
    h = hll_words(ctx.hll_new(p0), canon)
    est = h.estimate()
    lb = h.sketch_log2_blocks()
    print(f"n_reads {n:.0e} k={k}: windows {win:.3e}, distinct k-mers {n_distinct:.3e}, estimate at log2_regs {p0}: {est:.4e} "
          f"({(est - n_distinct) / n_distinct:+.3%}; standard error {1.04 / 2 ** (p0 / 2):.3%}); sketch sized log2_blocks {lb}", flush=True)
    sketch, regs = ctx.sketch_new(lb), ctx.hll_new(p0)
    with torch.cuda.stream(ctx.stream):
        t = medians([lambda: hll_words(regs, canon), lambda: sk_words(sketch, canon), lambda: dst.copy_(src),
                     lambda: hll_add(regs, bases, n, L, k), lambda: sk_add(sketch, bases, n, L, k)], reps)
    for nm, ms in zip(("hll_add_words", "sketch_add_words", "copy 8 B/key" if not two else "copy 16 B/key", "hll_add", "sketch_add"), t):
        print(f"  {nm:<18s} {ms:10.3f} ms {win / ms / 1e6:9.2f} Gkeys/s", flush=True)
    print(f"  sketch fill after the timed adds (saturating, repeated): {sketch.fill():.4f}", flush=True)
    del dst, sketch
    # routes: every log2_regs over all keys, registers warm (the steady state of a long input) and cold (zeroed before each add)
    n_cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    cap = n_cu * _lib.SKETCH_SWEEP_LANES_PER_CU // 256
    for p in (9, 14, 15, 18, 24):
        warm = hll_words(ctx.hll_new(p), canon)
        cold = ctx.hll_new(p)

        def cold_add():
            cold.regs.zero_()
            return hll_words(cold, canon)

        with torch.cuda.stream(ctx.stream):
            a, b = medians([lambda: hll_words(warm, canon), cold_add], reps)
        blocks = min(-(-win // 256), cap)
        route = "block-private" if p <= _lib.HLL_LDS_MAX_LOG2_REGS and win >= blocks * ((1 << p) >> 2) * _lib.HLL_LDS_KEYS_PER_DWORD else "global"
        print(f"  log2_regs {p:>2d} {route:<13s} warm {a:10.3f} ms {win / a / 1e6:9.2f} Gkeys/s   cold (with the memset) {b:10.3f} ms; "
              f"estimate {warm.estimate():.4e}", flush=True)
    cut = cap * ((1 << p0) >> 2) * _lib.HLL_LDS_KEYS_PER_DWORD
    if win > cut:
        below, at = src[:(cut - 1) * words], src[:cut * words]
        ra, rb = hll_words(ctx.hll_new(p0), below), hll_words(ctx.hll_new(p0), at)
        with torch.cuda.stream(ctx.stream):
            a, b = medians([lambda: hll_words(ra, below), lambda: hll_words(rb, at)], max(reps, 5))
        print(f"  log2_regs {p0} at the keys-per-block cut ({cut:.3e} keys): global {a:8.3f} ms {cut / a / 1e6:8.2f} Gkeys/s, "
              f"block-private {b:8.3f} ms {cut / b / 1e6:8.2f} Gkeys/s", flush=True)
    else:
        print(f"  log2_regs {p0}: {win:.3e} keys are below the keys-per-block cut ({cut:.3e}): the global route ran above", flush=True)


def main():
    from kmers_amd.api import Context

    args = sys.argv[1:]
    reps, k, ns = 3, 31, []
    while args:
        a = args.pop(0)
        if a == "--reps":
            reps = int(args.pop(0))
        elif a == "--k":
            k = int(args.pop(0))
        else:
            ns.append(int(float(a)))
    ctx = Context(0)
    ctx.set_work_buffer_limit(48 << 30)
    print(f"the distinct-key estimator beside the counting sketch and a plain copy; uniform reads of {L} bp from a genome at 30x with 1% "
          f"substitutions; median of {reps} alternating wall-clock runs each (ms) after 1 warm-up call; Gkeys/s = windows / time; MI355X", flush=True)
    for n in ns or [200_000, 10_000_000]:
        bench(ctx, n, k, reps)
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
