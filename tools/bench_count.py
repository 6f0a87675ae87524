"""dev tool: kmx_count_canonical against the composition of already-pinned calls that gives the same table --
kmx_canonical_windows -> canon[flags & 1] -> torch.unique(sorted, return_counts) -- alternating the two in one process, so both
see the same device state.  Both are checked equal on every shape before anything is timed.  Times are wall-clock medians of
synchronised calls (the count is synchronous: its answer comes back to the host).  Output: profiles/r07_count_bench.txt.
  python tools/bench_count.py [n_reads, default 1e7] [reps, default 5]

Bytes per window are a MODEL of the count's traffic, not a counter reading: windows written (9), the level-0 count and scatter
(9 + 9 + 8), each further level (8 + 8 + 8), the leaf (8 read, up to 17 written), the keep mask (1 + 1), the table's copy.  The
model covers random keys and a single key; the mixed heavy-hitter shape (90 % of the reads one k-mer) has none ("n/a")."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from kmers_amd.api import Context

LEAF = 4096


def levels(n_valid, k):
    """partition levels random keys need before every partition fits a leaf (8 bits each, at most ceil(2k / 8))"""
    lv, part = 1, n_valid / 256.0
    while part > LEAF and lv * 8 < 2 * k:
        lv += 1
        part /= 256.0
    return lv


def bytes_per_window(n_win, n_valid, n_distinct, k, heavy=False):
    v = n_valid / max(n_win, 1)
    b = 9.0 + 9.0 + 1.0                      # windows written; level-0 count reads canon + flags; the keep mask cleared
    if heavy:
        return b                              # one key: the count pass is the answer (no scatter, no leaf)
    b += 9.0 + 8.0 * v                       # level-0 scatter
    b += (levels(n_valid, k) - 1) * 24.0 * v  # further levels: count, scatter (read + write)
    d = n_distinct / max(n_win, 1)
    b += 8.0 * v + 17.0 * d                  # leaves: keys in; distinct keys, counts, keep bytes out
    b += v + 1.0 * v + 32.0 * d              # compaction: keep read twice, the table read and written
    return b


def composition(ctx, bases, n, L, k, offsets, host_offsets):
    w = ctx.canonical_windows(bases, n, L, k, offsets=offsets, host_offsets=host_offsets, want=("canon", "flags"))
    keys = w["canon"][(w["flags"] & 1) != 0]
    del w
    uk, uc = torch.unique(keys, sorted=True, return_counts=True)
    return uk, uc


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = Context(0)
    rng = np.random.default_rng(11)
    L = 150
    print(f"kmx_count_canonical vs kmx_canonical_windows -> mask -> torch.unique(return_counts); {n:.0e} reads; median of {reps} "
          f"alternating wall-clock runs each (ms); MI355X")
    print(f"{'shape':<36s} {'windows':>10s} {'distinct':>11s} {'count ms':>9s} {'comp ms':>9s} {'ratio':>6s} "
          f"{'count e9 k-mers/s':>18s} {'model B/win':>11s}")
    shapes = []
    base = ctx.gen_reads(n * L, seed=0xC0FFEE)
    shapes.append(("150 bp, k = 31", base, n, L, 31, None, None, False))
    shapes.append(("150 bp, k = 21", base, n, L, 21, None, None, False))
    dirty = base.clone()
    g = torch.Generator(device=ctx.device).manual_seed(3)
    rows = torch.nonzero(torch.rand(n, device=ctx.device, generator=g) < 0.02).flatten()
    dirty[rows * L + torch.randint(0, L, (rows.numel(),), device=ctx.device, generator=g)] = ord("N")
    shapes.append(("150 bp, k = 31, 2 % dirty reads", dirty, n, L, 31, None, None, False))
    lens = rng.integers(100, 161, n).astype(np.uint64)
    h_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    rag = ctx.gen_reads(int(h_off[-1]), seed=0xBEEF)
    d_off = ctx.to_device(h_off)
    shapes.append(("100-160 bp ragged, k = 31", rag, n, 160, 31, d_off, h_off, False))
    mixed = base.clone()
    mixed.view(n, L)[torch.rand(n, device=ctx.device, generator=g) < 0.9] = ord("A")
    shapes.append(("150 bp, 90 % of reads all A, k = 31", mixed, n, L, 31, None, None, None))
    polya = torch.full((n * L,), ord("A"), dtype=torch.uint8, device=ctx.device)
    shapes.append(("150 bp all A (one k-mer), k = 31", polya, n, L, 31, None, None, True))
    for name, bases, nr, Lr, k, off, hoff, heavy in shapes:
        ct = lambda: ctx.count_canonical(bases, nr, Lr, k, offsets=off)   # noqa: E731
        cp = lambda: composition(ctx, bases, nr, Lr, k, off, hoff)        # noqa: E731
        _, (km, cnt) = timed(ct)
        _, (uk, uc) = timed(cp)
        same = uk.numel() == km.numel() and torch.equal(uk, km) and torch.equal(uc, cnt)
        n_valid = int(cnt.sum().item())
        n_distinct = int(km.numel())
        n_win = int(hoff is None and nr * (Lr - k + 1) or int(np.maximum(lens.astype(np.int64) - k + 1, 0).sum()))
        del km, cnt, uk, uc
        if not same:
            print(f"{name:<36s} MISMATCH: the count and the composition give different tables; not timed")
            continue
        tc, tp = [], []
        for _ in range(reps):
            t, o = timed(ct)
            tc.append(t)
            del o
            t, o = timed(cp)
            tp.append(t)
            del o
        mc, mp = statistics.median(tc), statistics.median(tp)
        print(f"{name:<36s} {n_win:>10.3e} {n_distinct:>11.4e} {mc:9.2f} {mp:9.2f} {mp / mc:6.2f} {n_win / mc / 1e6:18.2f} "
              + (f"{bytes_per_window(n_win, n_valid, n_distinct, k, heavy):11.1f}" if heavy is not None else f"{'n/a':>11s}"))
        torch.cuda.empty_cache()
    held, allocs = ctx.work_buffer_info()
    print(f"work buffer held at the end: {held / 2**30:.2f} GiB ({allocs} allocations)")
    ctx.close()


if __name__ == "__main__":
    main()
