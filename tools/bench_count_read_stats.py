"""dev tool: kmx_count_read_stats(2) beside what a caller had before it, alternating in one process so all see the same device state;
each pair is checked equal before anything is timed.
  uniform reads  vs count_lookup_reads(2) -> reshape (n, W) -> torch min / max / sum / kthvalue(dim=1) and the two counts.  The
                 composition has no flags: a window with an invalid byte reads as count 0 there, so only the rows of reads without one
                 are compared (all of them on clean input), and it has no span at all.  kthvalue(W // 2 + 1) is the upper median the
                 call reports (torch.median takes the lower one of an even number; same kernel, same cost).
  ragged reads   torch has no segmented median or longest run: count_lookup_reads alone (window offsets made beforehand) is the floor
                 the call cannot beat.
`lookup ms` is count_lookup_reads(2) on the same input in every row: call ms - lookup ms is what the statistics cost.  Times are
wall-clock medians of synchronised calls (ms).  Output: profiles/r12_count_read_stats_bench.txt.
  python tools/bench_count_read_stats.py [n_reads, default 1e7] [reps, default 3]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from kmers_amd import _lib
from kmers_amd.api import Context


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def composition(lookup, n, W, solid_min):
    """columns N_PRESENT .. MEDIAN of the rows, from the per-window counts alone"""
    c = lookup().view(n, W)
    return torch.stack([(c != 0).sum(1), (c >= solid_min).sum(1), c.min(1).values, c.max(1).values, c.sum(1),
                        c.kthvalue(W // 2 + 1, dim=1).values], dim=1)


def race(name, call, lookup, comp, reps, n_win, W=0):
    """check equal, then alternate the three; prints one row"""
    _, rows = timed(call)
    if comp is not None:
        _, ref = timed(comp)
        clean = rows[:, _lib.RS_N_VALID] == W
        same = torch.equal(rows[clean][:, _lib.RS_N_PRESENT:_lib.RS_MEDIAN + 1], ref[clean])
        checked = int(clean.sum().item())
        del ref
        if not same or checked == 0:
            print(f"{name:<44s} MISMATCH: the call and its composition differ; not timed")
            return
    del rows
    t = {"call": [], "lookup": [], "comp": []}
    for _ in range(reps):
        for key, f in (("call", call), ("lookup", lookup), ("comp", comp)):
            if f is not None:
                ms, o = timed(f)
                t[key].append(ms)
                del o
    mc, ml = statistics.median(t["call"]), statistics.median(t["lookup"])
    spread = (max(t["call"]) - min(t["call"])) / mc
    if comp is not None:
        mp = statistics.median(t["comp"])
        tail = f"{mp:9.2f} {mp / mc:6.2f}"
    else:
        tail = f"{'-':>9s} {'-':>6s}"
    print(f"{name:<44s} {n_win:>10.3e} {mc:9.2f} {ml:9.2f} {mc - ml:9.2f} {(mc - ml) * 1e6 / n_win:8.4f} {tail} {spread:7.2f}")
    torch.cuda.empty_cache()


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    ctx = Context(0)
    rng = np.random.default_rng(12)
    L, sm = 150, 2
    print(f"count_read_stats(2) beside count_lookup_reads(2) and the torch composition over its output; {n:.0e} reads, solid_min = {sm}; "
          f"median of {reps} alternating wall-clock runs each (ms); stats = call - lookup; spread = (max - min) / median of the call's runs; MI355X")
    print(f"{'shape':<44s} {'windows':>10s} {'call ms':>9s} {'lookup ms':>9s} {'stats ms':>9s} {'ns/win':>8s} {'comp ms':>9s} {'ratio':>6s} {'spread':>7s}")
    g = torch.Generator(device=ctx.device).manual_seed(5)
    # reads drawn from a genome at 7.5-fold coverage: counts above 1, so that the select has bits to walk
    genome = ctx.gen_reads(max(100_000, 20 * n), seed=0xC0FFEE)

    def draw(nr, Lr):
        reads = ctx.empty(nr * Lr, torch.uint8)
        for r0 in range(0, nr, 1_000_000):                      # (in pieces: the gather's index is 8 bytes per base)
            m = min(1_000_000, nr - r0)
            starts = torch.randint(0, genome.numel() - Lr + 1, (m,), device=ctx.device, generator=g)
            reads[r0 * Lr:(r0 + m) * Lr] = genome[(starts[:, None] + torch.arange(Lr, device=ctx.device)[None, :]).reshape(-1)]
        return reads

    a = draw(n, L)

    def uniform_row(tag, k, bases, nr, Lr, table):
        one = k <= 31
        km, cnt = table
        W = Lr - k + 1
        stats = ctx.count_read_stats if one else ctx.count_read_stats2
        look = ctx.count_lookup_reads if one else ctx.count_lookup_reads2
        out = ctx.empty(8 * nr, torch.int64)
        win = ctx.empty(nr * W, torch.int64)
        call = lambda: stats(bases, nr, Lr, k, km, cnt, solid_min=sm, out=out)
        lookup = lambda: look(bases, nr, Lr, k, km, cnt, out=win)
        race(tag, call, lookup, lambda: composition(lookup, nr, W, sm), reps, nr * W, W)

    km, cnt = ctx.count_canonical(a, n, L, 31)
    uniform_row("150 bp, k = 31, own table", 31, a, n, L, (km, cnt))
    dirty = a.clone()
    rows = torch.nonzero(torch.rand(n, device=ctx.device, generator=g) < 0.02).flatten()
    dirty[rows * L + torch.randint(0, L, (rows.numel(),), device=ctx.device, generator=g)] = ord("N")
    uniform_row("150 bp, k = 31, 2 % dirty reads", 31, dirty, n, L, (km, cnt))
    del dirty
    nsm = min(100_000, n)
    uniform_row("150 bp, k = 31, 1e5 reads, the large table", 31, a[:nsm * L], nsm, L, (km, cnt))
    # ragged reads: the floor is the lookup alone
    lens = rng.integers(100, 161, n).astype(np.uint64)
    h_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    rag = ctx.gen_reads(int(h_off[-1]), seed=0xFACE)
    m = min(a.numel(), rag.numel())
    rag[:m] = a[:m]                                             # (mostly k-mers of the table)
    d_off = ctx.to_device(h_off)
    wo = ctx.to_device(ctx.win_offsets(n, 160, 31, h_off))
    out = ctx.empty(8 * n, torch.int64)
    win = ctx.empty(int(ctx.win_offsets(n, 160, 31, h_off)[-1]), torch.int64)
    race("100-160 bp ragged, k = 31", lambda: ctx.count_read_stats(rag, n, 160, 31, km, cnt, solid_min=sm, offsets=d_off, out=out),
         lambda: ctx.count_lookup_reads(rag, n, 160, 31, km, cnt, offsets=d_off, win_offsets=wo, out=win), None, reps, win.numel())
    del rag, out, win, wo, d_off, km, cnt
    torch.cuda.empty_cache()
    n2 = min(n, 5_000_000)                                      # (the two-word counter's working set: 36 bytes per window)
    table2 = ctx.count_canonical2(a[:n2 * L], n2, L, 47)
    uniform_row(f"150 bp, k = 47, {n2:.0e} reads, own table", 47, a[:n2 * L], n2, L, table2)
    del table2
    torch.cuda.empty_cache()
    nl, Ll = min(100_000, n), 1000
    long_reads = draw(nl, Ll)
    uniform_row("1000 bp, k = 31, 1e5 reads, own table", 31, long_reads, nl, Ll, ctx.count_canonical(long_reads, nl, Ll, 31))
    held, allocs = ctx.work_buffer_info()
    print(f"work buffer held at the end: {held / 2**30:.2f} GiB ({allocs} allocations)")
    ctx.close()


if __name__ == "__main__":
    main()
