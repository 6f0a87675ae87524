"""dev tool: kmx_count_canonical2 (two-word k-mers, k = 33..64) against the only composition of pinned calls that gives the same
table -- kmx_canonical_windows2 -> canon2[flags & 1] -> both words XOR 1 << 63 -> stable torch.sort by the low word, then stable by
the high word -> run heads and lengths -- alternating the two in one process, so both see the same device state.  Both are checked
equal on every shape before anything is timed.  Times are wall-clock medians of synchronised calls (the count is synchronous).
kmx_count_canonical at k = 31 on the same reads, in the same run, is the yardstick for what the second word costs.
Output: profiles/r08_count2_bench.txt.
  python tools/bench_count2.py [n_reads, default 5e6] [reps, default 5] [--count-only]

Bytes per window are a MODEL of the count's traffic, not a counter reading: windows written (17), the level-0 count
(17) and scatter (17 + 16), each further level (16 + 16 + 16), the leaf (16 read, up to 33 written: key, count slot, mark), the
keep mask (1 + 1), the table's copy.  The mixed heavy-hitter shape has no model ("n/a")."""
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
SIGN = torch.iinfo(torch.int64).min


def levels(n_valid, k):
    """partition levels random keys need before every partition fits a leaf (8 bits each, at most ceil(2k / 8))"""
    lv, part = 1, n_valid / 256.0
    while part > LEAF and lv * 8 < 2 * k:
        lv += 1
        part /= 256.0
    return lv


def bytes_per_window(n_win, n_valid, n_distinct, k, heavy=False):
    v = n_valid / max(n_win, 1)
    b = 17.0 + 17.0 + 1.0                     # windows written; level-0 count reads canon2 + flags; the keep mask cleared
    if heavy:
        return b                              # one key: the count pass is the answer (no scatter, no leaf)
    b += 17.0 + 16.0 * v                      # level-0 scatter
    b += (levels(n_valid, k) - 1) * 48.0 * v  # further levels: count, scatter (read + write)
    d = n_distinct / max(n_win, 1)
    b += 16.0 * v + 33.0 * d                  # leaves: keys in; distinct keys, count slots, keep bytes out
    b += v + 1.0 * v + 48.0 * d               # compaction: keep read twice, the table read and written
    return b


def composition(ctx, bases, n, L, k, offsets, host_offsets):
    w = ctx.canonical_windows2(bases, n, L, k, offsets=offsets, host_offsets=host_offsets)
    del w["fw"], w["rc"]
    valid = (w["flags"] & 1) != 0
    canon = w["canon"].view(-1, 2)
    # (each word masked, sorted and gathered as a dense 1-D array of its own: a row gather of the (N, 2) tensor by 1e8 and more
    # indices came back wrong from torch 2.10 on ROCm 7.0; XOR 1 << 63: signed order = unsigned order)
    lo = canon[:, 0][valid] ^ SIGN
    hi = canon[:, 1][valid] ^ SIGN
    del w, canon, valid
    p = torch.sort(lo, stable=True).indices
    lo, hi = lo[p], hi[p]
    p = torch.sort(hi, stable=True).indices
    lo, hi = lo[p], hi[p]
    del p
    head = torch.ones(lo.numel(), dtype=torch.bool, device=lo.device)
    head[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    idx = torch.nonzero(head).flatten()
    uc = torch.diff(idx, append=torch.tensor([lo.numel()], device=lo.device))
    return torch.stack((lo[idx], hi[idx]), dim=1) ^ SIGN, uc


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    count_only = "--count-only" in sys.argv        # (for a kernel trace: the composition's kernels stay out of it)
    n = int(float(args[0])) if len(args) > 0 else 5_000_000
    reps = int(args[1]) if len(args) > 1 else 5
    ctx = Context(0)
    rng = np.random.default_rng(11)
    L = 150
    print(f"kmx_count_canonical2 vs kmx_canonical_windows2 -> mask -> two stable torch.sort -> run lengths; {n:.0e} reads; median of "
          f"{reps} alternating wall-clock runs each (ms); MI355X")
    print(f"{'shape':<36s} {'windows':>10s} {'distinct':>11s} {'count ms':>9s} {'min..max':>15s} {'comp ms':>9s} {'ratio':>6s} "
          f"{'count e9 k-mers/s':>18s} {'ns/window':>9s} {'model B/win':>11s}")
    shapes = []
    base = ctx.gen_reads(n * L, seed=0xC0FFEE)
    shapes.append(("150 bp, k = 31 (one word)", base, n, L, 31, None, None, False))
    shapes.append(("150 bp, k = 47", base, n, L, 47, None, None, False))
    shapes.append(("150 bp, k = 63", base, n, L, 63, None, None, False))
    shapes.append(("150 bp, k = 33", base, n, L, 33, None, None, False))
    dirty = base.clone()
    g = torch.Generator(device=ctx.device).manual_seed(3)
    rows = torch.nonzero(torch.rand(n, device=ctx.device, generator=g) < 0.02).flatten()
    dirty[rows * L + torch.randint(0, L, (rows.numel(),), device=ctx.device, generator=g)] = ord("N")
    shapes.append(("150 bp, k = 47, 2 % dirty reads", dirty, n, L, 47, None, None, False))
    lens = rng.integers(100, 161, n).astype(np.uint64)
    h_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    rag = ctx.gen_reads(int(h_off[-1]), seed=0xBEEF)
    d_off = ctx.to_device(h_off)
    shapes.append(("100-160 bp ragged, k = 47", rag, n, 160, 47, d_off, h_off, False))
    mixed = base.clone()
    mixed.view(n, L)[torch.rand(n, device=ctx.device, generator=g) < 0.9] = ord("A")
    shapes.append(("150 bp, 90 % of reads all A, k = 47", mixed, n, L, 47, None, None, None))
    polya = torch.full((n * L,), ord("A"), dtype=torch.uint8, device=ctx.device)
    shapes.append(("150 bp all A (one k-mer), k = 47", polya, n, L, 47, None, None, True))
    for name, bases, nr, Lr, k, off, hoff, heavy in shapes:
        one_word = k <= 31
        ct = (lambda: ctx.count_canonical(bases, nr, Lr, k, offsets=off)) if one_word else (lambda: ctx.count_canonical2(bases, nr, Lr, k, offsets=off))
        cp = lambda: composition(ctx, bases, nr, Lr, k, off, hoff)        # noqa: E731
        _, (km, cnt) = timed(ct)
        n_valid = int(cnt.sum().item())
        n_distinct = int(cnt.numel())
        n_win = int(hoff is None and nr * (Lr - k + 1) or int(np.maximum(lens.astype(np.int64) - k + 1, 0).sum()))
        compare = not (one_word or count_only)
        if compare:
            _, (uk, uc) = timed(cp)
            same = tuple(uk.shape) == tuple(km.shape) and torch.equal(uk, km) and torch.equal(uc, cnt)
            del uk, uc
            if not same:
                print(f"{name:<36s} MISMATCH: the count and the composition give different tables; not timed")
                continue
        del km, cnt
        tc, tp = [], []
        for _ in range(reps):
            t, o = timed(ct)
            tc.append(t)
            del o
            if compare:
                t, o = timed(cp)
                tp.append(t)
                del o
        mc = statistics.median(tc)
        mp = statistics.median(tp) if tp else float("nan")
        model = bytes_per_window(n_win, n_valid, n_distinct, k, heavy) if heavy is not None and not one_word else None
        print(f"{name:<36s} {n_win:>10.3e} {n_distinct:>11.4e} {mc:9.2f} {min(tc):7.2f}..{max(tc):<7.2f}"
              f"{mp:9.2f} {mp / mc:6.2f} {n_win / mc / 1e6:18.2f} {mc * 1e6 / n_win:9.3f} "
              + (f"{model:11.1f}" if model is not None else f"{'n/a':>11s}"), flush=True)
        torch.cuda.empty_cache()
    held, allocs = ctx.work_buffer_info()
    print(f"work buffer held at the end: {held / 2**30:.2f} GiB ({allocs} allocations)")
    ctx.close()


if __name__ == "__main__":
    main()
