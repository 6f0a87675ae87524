"""dev tool: kmx_count_read_paths(2) beside its only composition, alternating in one process so both see the same device state; the two
are checked equal before anything is timed.
  composition  count_lookup_reads(2) with the places as the counts (8 bytes per window out), the flags of canonical_windows(2), then
               torch on the device: shifts and compares over the flat window array for "continues its predecessor", nonzero for
               the heads and the tails, searchsorted for the unitig of every head, a cumsum for the reads' offsets.
  call         count_read_paths(2) with the index made once up front and room for the segments known (one call, no counting pass).
The table is count_canonical(2) of the batch itself -- reads drawn from a genome at 7.5-fold coverage, 0.5 % of their bases
substituted, so the graph has tips and bubbles -- and the unitigs are the batch's own (min_count = 1: every window is mapped).  Times
are wall-clock medians of synchronised calls (ms).  Bytes follow DESIGN 4.6.7: per window what the call moves after the windows
pass, per segment what the emit adds.  Output: profiles/count_read_paths_bench.txt.
  python tools/bench_read_paths.py [n_reads, default 1e7] [reps, default 3]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from kmers_amd.api import Context


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def composition(ctx, reads, n, L, k, km, place, unitig_offsets):
    """-> path offsets int64[n + 1], segments int64[S, 4], from the definitions of include/kmx.h (uniform reads)"""
    one = k <= 31
    W = L - k + 1
    pl = (ctx.count_lookup_reads if one else ctx.count_lookup_reads2)(reads, n, L, k, km, place)
    flags = (ctx.canonical_windows(reads, n, L, k, want=("flags",)) if one else ctx.canonical_windows2(reads, n, L, k))["flags"]
    dev = pl.device
    mapped = pl != 0
    p = (pl >> 3) - 1
    d = (1 - ((flags.to(torch.int64) >> 1) & 1)) ^ (pl & 1)
    del flags
    j = torch.arange(pl.numel(), device=dev)
    cont = torch.zeros_like(mapped)
    fwd = (p[1:] == p[:-1] + 1) & ((pl[1:] & 2) == 0)
    rev = (p[1:] + 1 == p[:-1]) & ((pl[1:] & 4) == 0)
    cont[1:] = mapped[1:] & mapped[:-1] & (d[1:] == d[:-1]) & torch.where(d[1:] == 0, fwd, rev) & (j[1:] % W != 0)
    del fwd, rev
    head = mapped & ~cont
    tail = mapped.clone()
    tail[:-1] &= ~cont[1:]
    hj, tj = torch.nonzero(head)[:, 0], torch.nonzero(tail)[:, 0]
    csum = torch.cumsum(head, 0)
    po = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), csum[W - 1::W]])
    del csum, head, tail, cont, mapped, j
    ph = p[hj]
    u = torch.searchsorted(unitig_offsets, ph, right=True) - 1
    segs = torch.stack([hj // W, ((tj - hj + 1) << 32) | (hj % W), u, ((ph - unitig_offsets[u]) << 1) | d[hj]], 1)
    return po, segs


def race(ctx, name, reads, n, L, k, reps):
    one = k <= 31
    km, cnt = (ctx.count_canonical if one else ctx.count_canonical2)(reads, n, L, k)
    un = (ctx.count_unitigs if one else ctx.count_unitigs2)(km, cnt, k, 1)
    n_tab = cnt.numel()
    place = ctx.count_unitig_index(un, n_tab)
    paths = ctx.count_read_paths if one else ctx.count_read_paths2
    _, a = timed(lambda: paths(reads, n, L, k, km, un, place=place))
    S = a.n_segments
    call = lambda: paths(reads, n, L, k, km, un, place=place, max_segments=S)
    comp = lambda: composition(ctx, reads, n, L, k, km, place, un.offsets)
    _, b = timed(comp)
    if not (torch.equal(a.offsets, b[0]) and torch.equal(a.segments, b[1])):
        print(f"{name:<28s} MISMATCH: the call and its composition differ; not timed")
        return
    del a, b
    t = {"call": [], "comp": []}
    for _ in range(reps):
        for key, f in (("call", call), ("comp", comp)):
            ms, o = timed(f)
            t[key].append(ms)
            del o
    mc, mp = statistics.median(t["call"]), statistics.median(t["comp"])
    spread = (max(t["call"]) - min(t["call"])) / mc
    n_win = n * (L - k + 1)
    words = 1 if one else 2
    per_window = L / (L - k + 1) + 8 * words + 1 + (8 * words + 1 + 8) + (8 + 1) + 20 / 64   # bases; windows out; lookup in, out; mark in, out
    print(f"{name:<28s} {n_tab:>10.3e} {un.n_unitigs:>10.3e} {n_win:>10.3e} {S:>10.3e} {S / n:>8.2f} {mc:9.2f} {n_win / mc / 1e6:9.2f} {mp:9.2f} {mp / mc:6.2f} "
          f"{spread:7.2f}   model bytes/window {per_window:.1f} (+ the lookup's gathers), bytes/segment {32 + 8 + 1 + 24}")
    torch.cuda.empty_cache()


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    ctx = Context(0)
    L = 150
    print(f"count_read_paths(2) beside count_lookup_reads(2) on the places + the windows' flags + torch compares, nonzero, searchsorted and cumsum; "
          f"{n:.0e} reads of {L} bp against the batch's own unitigs; median of {reps} alternating wall-clock runs each (ms); Gwin/s = windows / "
          f"call ms; ratio = comp / call; spread = (max - min) / median of the call's runs; MI355X")
    print(f"{'batch':<28s} {'entries':>10s} {'unitigs':>10s} {'windows':>10s} {'segments':>10s} {'seg/read':>8s} {'call ms':>9s} {'Gwin/s':>9s} {'comp ms':>9s} "
          f"{'ratio':>6s} {'spread':>7s}")
    g = torch.Generator(device=ctx.device).manual_seed(5)
    genome = ctx.gen_reads(max(100_000, 20 * n), seed=0xC0FFEE)
    reads = ctx.empty(n * L, torch.uint8)
    for r0 in range(0, n, 1_000_000):                      # (in pieces: the gather's index is 8 bytes per base)
        m = min(1_000_000, n - r0)
        starts = torch.randint(0, genome.numel() - L + 1, (m,), device=ctx.device, generator=g)
        piece = genome[(starts[:, None] + torch.arange(L, device=ctx.device)[None, :]).reshape(-1)]
        sub = torch.rand(piece.numel(), device=ctx.device, generator=g) < 0.005
        piece[sub] = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=ctx.device)[torch.randint(0, 4, (int(sub.sum()),), device=ctx.device, generator=g)]
        reads[r0 * L:(r0 + m) * L] = piece
    del genome
    race(ctx, "k = 31", reads, n, L, 31, reps)
    n2 = min(n, 5_000_000)                                 # (the two-word counter's working set: 36 bytes per window)
    race(ctx, f"k = 47, {n2:.0e} reads", reads[:n2 * L], n2, L, 47, reps)
    held, allocs = ctx.work_buffer_info()
    print(f"work buffer held at the end: {held / 2**30:.2f} GiB ({allocs} allocations)")
    ctx.close()


if __name__ == "__main__":
    main()
