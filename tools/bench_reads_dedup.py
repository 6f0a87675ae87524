"""dev tool: kmx_reads_dedup beside a torch composition that yields the same keep bytes, and beside a plain copy of the bytes it reads.
One process, so that everything sees the same device state; the call and its composition are checked equal before anything is
timed.
  (a)  call: Context.reads_dedup on uniform reads of 150 bp, no strand, no score: keys, the two-word counter's sort, groups, verify.
  (b)  comp: torch on the device: the bases packed two bits each into five int64 words per read, torch.unique(dim=0) with the
       inverse, the first read of every class by scatter_reduce(amin): keep[r] = (first[inverse[r]] == r).
  (c)  copy: Tensor.copy_ of the batch's bytes (as many as the key kernel reads, and as many written).
Reads are upper-case ACGT, which is what lets the composition pack them.  A share of the reads are copies of other reads of the
batch that are no copies themselves, drawn uniformly (classes of two, three, a few more); the last shape instead makes 1 % of the
batch copies of ONE read: a class the sort has to take through all 16 digits, one host round trip each.  Times are wall-clock medians of synchronised calls (ms) after three
warm-up calls of each, the contestants alternating.  The split of (a) into key / sort / groups / verify is device time of the
kernels of one more call under torch.profiler, summed by kernel name; `host` is the call's wall-clock median minus their sum: the
sort's round trips to the host, launches and the work buffer.
Output: profiles/reads_dedup_bench.txt.
  python tools/bench_reads_dedup.py [n_reads, default 1e7] [reps, default 5]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from tools.bench_reads_adapter import median_ms, timed

L = 150
WORDS = (L + 31) // 32


def make_reads(ctx, n, dup_share, one_class, g):
    """-> uint8[n * L]: read r is a copy of base read idx[r]; idx[r] = r but for the duplicates"""
    dev = ctx.device
    base = ctx.gen_reads(n * L, seed=0xD0D0).view(n, L)
    idx = torch.arange(n, device=dev)
    dup = torch.rand(n, device=dev, generator=g) < dup_share
    originals = torch.nonzero(~dup).squeeze(1)   # (a duplicate copies a read that is no duplicate itself: the share dropped is the share made)
    n_dup = n - originals.numel()
    idx[dup] = originals[0] if one_class else originals[torch.randint(0, originals.numel(), (n_dup,), device=dev, generator=g)]
    return base[idx].reshape(-1)


def keep_comp(bases, n):
    """uniform reads [n, L] of upper-case ACGT -> keep bytes of a first-occurrence dedup"""
    dev = bases.device
    code = torch.zeros(256, dtype=torch.int64, device=dev)
    code[list(b"ACGT")] = torch.arange(4, device=dev)
    shift = 2 * (torch.arange(L, device=dev) % 32)
    packed = torch.zeros(n, WORDS, dtype=torch.int64, device=dev)
    for a in range(0, n, 1 << 20):   # (a chunk of reads at a time: the codes as int64 are eight times the batch)
        c = code[bases[a * L:(a + (1 << 20)) * L].view(-1, L).long()] << shift
        for w in range(WORDS):
            packed[a:a + c.shape[0], w] = c[:, 32 * w:32 * (w + 1)].sum(1)
    _, inverse = torch.unique(packed, dim=0, return_inverse=True)
    first = torch.full((int(inverse.max()) + 1,), n, dtype=torch.int64, device=dev)
    first.scatter_reduce_(0, inverse, torch.arange(n, device=dev), "amin")
    return (first[inverse] == torch.arange(n, device=dev)).to(torch.uint8)


def split_ms(call):
    """device time of one call's kernels by step (ms), or None where the profiler gives none"""
    try:
        from torch.profiler import ProfilerActivity, profile

        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        steps = {"key": 0.0, "sort": 0.0, "groups": 0.0, "verify": 0.0}
        seen = False
        for ev in prof.key_averages():
            us = getattr(ev, "device_time_total", None)
            if us is None:
                us = getattr(ev, "cuda_time_total", 0.0)
            if not us:
                continue
            name = ev.key
            if "reads_dedup_key" in name:
                steps["key"] += us
            elif "reads_dedup_verify" in name or "reads_dedup_summary" in name:
                steps["verify"] += us
            elif "reads_dedup_head" in name or "scan_single" in name:
                steps["groups"] += us   # (the sort's own one-block scan, once per call, lands here too: microseconds)
            elif "kmx" in name:
                steps["sort"] += us
            else:
                continue
            seen = True
        return {k: v / 1e3 for k, v in steps.items()} if seen else None
    except Exception as exc:   # noqa: BLE001  (a measurement aid: the race above stands without it)
        print(f"(no split: {type(exc).__name__}: {exc})")
        return None


def race(ctx, name, bases, n, reps):
    call = lambda: ctx.reads_dedup(bases, n, L)   # noqa: E731
    comp = lambda: keep_comp(bases, n)            # noqa: E731
    _, d = timed(call)
    _, want = timed(comp)
    same = torch.equal(d.keep, want)
    kept, largest, collisions = d.kept, d.largest, d.collisions
    del d, want
    torch.cuda.empty_cache()
    if not same:
        print(f"{name:<10s} MISMATCH: the call and its composition differ; not timed")
        return
    dst = torch.empty_like(bases)
    copy = lambda: dst.copy_(bases)               # noqa: E731
    with torch.cuda.stream(ctx.stream):
        (a, b, c), spread = median_ms([call, comp, copy], reps)
        s = split_ms(call)
    nb = bases.numel()
    split = (f"{s['key']:8.3f} {s['sort']:8.3f} {s['groups']:8.3f} {s['verify']:8.3f} {a - sum(s.values()):8.3f}" if s
             else " ".join(f"{'-':>8s}" for _ in range(5)))
    print(f"{name:<10s} {n:>10.3e} {1 - kept / n:7.3f} {largest:>8d} {collisions:>5d} {a:9.3f} {n / a / 1e3:8.2f} {nb / a / 1e6:8.1f} {split} {b:10.3f} "
          f"{b / a:7.2f} {c:8.3f} {a / c:7.2f} {spread[0]:7.2f}")
    del dst
    torch.cuda.empty_cache()


def main():
    from kmers_amd.api import Context

    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = Context(0)
    print(f"reads_dedup beside a torch composition of the same keep bytes (2-bit packing, torch.unique(dim=0), first of every class) and a plain copy "
          f"of the batch's bytes; {n:.0e} uniform reads of {L} bp, no strand, no score, hash_bits = 64; median of {reps} alternating wall-clock runs each "
          f"(ms) after 3 warm-up calls; call = Context.reads_dedup, Mreads/s = reads / time, GB/s = the batch's bytes / time; key, sort, groups, verify = "
          f"device time of the kernels of one more call by step (torch.profiler), host = call minus their sum (the sort's round trips, launches); comp = "
          f"the torch composition, b/a = comp / call; copy = Tensor.copy_ of the batch's bytes, a/c = call / copy; dropped = share of the reads "
          f"dropped, largest = the largest class; spread = (max - min) / median of the call's runs; MI355X")
    print(f"{'batch':<10s} {'reads':>10s} {'dropped':>7s} {'largest':>8s} {'coll':>5s} {'call':>9s} {'Mreads/s':>8s} {'GB/s':>8s} {'key':>8s} {'sort':>8s} "
          f"{'groups':>8s} {'verify':>8s} {'host':>8s} {'comp':>10s} {'b/a':>7s} {'copy':>8s} {'a/c':>7s} {'spread':>7s}")
    g = torch.Generator(device=ctx.device).manual_seed(18)
    for name, share, one in (("0 % dup", 0.0, False), ("10 % dup", 0.10, False), ("50 % dup", 0.50, False), ("1 % class", 0.01, True)):
        bases = make_reads(ctx, n, share, one, g)
        race(ctx, name, bases, n, reps)
        del bases
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
