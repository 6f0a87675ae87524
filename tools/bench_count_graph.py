"""dev tool: kmx_count_adjacency(2) beside what a caller had before it, alternating in one process so both see the same device state;
the two are checked equal before anything is timed.
  composition  eight query arrays made with torch shifts (S_c and P_c of every key), canonicalised -- kmx_canonical_words for
               one-word keys; two-word keys have no such call, so the 128-bit reverse complement is spelled in torch as well --
               then kmx_count_lookup(2) per slot and the fold of the eight answers into the edge byte.  Eight full-size temporaries
               and eight independent searches per entry.
  call         count_adjacency(2) with the edge bytes alone (what the composition produces), and with flips and neighbour indices.
The table is count_canonical(2) of reads drawn from a genome at 7.5-fold coverage.  Times are wall-clock medians of synchronised
calls (ms).  Output: profiles/count_graph_bench.txt.
  python tools/bench_count_graph.py [n_reads, default 1e7] [reps, default 3]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from kmers_amd.api import Context

M64 = -1   # all ones as an int64


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def lsr(x, s):
    """logical shift right of int64 words holding u64"""
    return (x >> s) & ((1 << (64 - s)) - 1) if s else x


def _revgroups64(x):
    for s, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        x = (lsr(x, s) & m) | ((x & m) << s)
    return lsr(x, 32) | (x << 32)


def canon2(lo, hi, k):
    """min(w, rc(w)) of two-word words, in torch: the reverse complement is the group reversal of the complement, shifted down"""
    rl, rh = _revgroups64(~hi), _revgroups64(~lo)
    s = 128 - 2 * k
    if s >= 64:
        rl, rh = lsr(rh, s - 64), torch.zeros_like(rh)
    elif s:
        rl, rh = lsr(rl, s) | (rh << (64 - s)), lsr(rh, s)
    # unsigned compare of int64 words: flip the sign bit
    sign = -(2**63)
    less = ((rh ^ sign) < (hi ^ sign)) | ((rh == hi) & ((rl ^ sign) < (lo ^ sign)))
    return torch.where(less, rl, lo), torch.where(less, rh, hi)


def composition(ctx, km, cnt, k, min_count):
    """the edge byte of every entry out of eight lookups"""
    one = k <= 31
    n = cnt.numel()
    edges = torch.zeros(n, dtype=torch.uint8, device=ctx.device)
    present = cnt >= min_count
    top = 2 * k - 2
    for e in range(8):
        c = e & 3
        if one:
            w = lsr(km, 2) | (c << top) if e < 4 else ((km << 2) | c) & ((1 << (2 * k)) - 1)
            q, _ = ctx.canonical_words(w, k)
            hit = ctx.count_lookup(km, cnt, k, q)
        else:
            lo, hi = km[:, 0], km[:, 1]
            if e < 4:
                wl, wh = lsr(lo, 2) | (hi << 62), lsr(hi, 2) | (c << (top - 64))
            else:
                wl, wh = (lo << 2) | c, ((hi << 2) | lsr(lo, 62)) & (((1 << (2 * k - 64)) - 1) if k < 64 else M64)
            ql, qh = canon2(wl, wh, k)
            hit = ctx.count_lookup2(km, cnt, k, torch.stack([ql, qh], dim=1))
        # (counts are u64 in int64 words: a count of 2^63 or more does not occur in these tables)
        edges |= ((present & (hit >= min_count)).to(torch.uint8) << e)
    return edges


def race(ctx, name, km, cnt, k, reps, min_count=1):
    adj = ctx.count_adjacency if k <= 31 else ctx.count_adjacency2
    n = cnt.numel()
    call = lambda: adj(km, cnt, k, min_count)
    full = lambda: adj(km, cnt, k, min_count, flips=True, neighbors=True)
    comp = lambda: composition(ctx, km, cnt, k, min_count)
    _, a = timed(call)
    _, b = timed(comp)
    if not torch.equal(a, b):
        print(f"{name:<40s} MISMATCH: the call and its composition differ; not timed")
        return
    hist = ctx.count_edge_histogram(a)
    del a, b
    t = {"call": [], "full": [], "comp": []}
    for _ in range(reps):
        for key, f in (("call", call), ("full", full), ("comp", comp)):
            ms, o = timed(f)
            t[key].append(ms)
            del o
    mc, mf, mp = (statistics.median(t[key]) for key in ("call", "full", "comp"))
    spread = (max(t["call"]) - min(t["call"])) / mc
    print(f"{name:<40s} {n:>10.3e} {mc:9.2f} {mc * 1e6 / n:8.3f} {mf:9.2f} {mp:9.2f} {mp / mc:6.2f} {spread:7.2f}   "
          f"edges/entry {hist.n_edges / max(n, 1):.2f}, interior {hist.n_interior / max(n, 1):.2f}")
    torch.cuda.empty_cache()


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    ctx = Context(0)
    L = 150
    print(f"count_adjacency(2) beside the composition of torch shifts, canonical words, eight count_lookup(2) and the bit fold; tables of "
          f"{n:.0e} reads of {L} bp; median of {reps} alternating wall-clock runs each (ms); call = edge bytes alone, full = with flips and "
          f"indices; ratio = comp / call; spread = (max - min) / median of the call's runs; MI355X")
    print(f"{'table':<40s} {'entries':>10s} {'call ms':>9s} {'ns/entry':>8s} {'full ms':>9s} {'comp ms':>9s} {'ratio':>6s} {'spread':>7s}")
    g = torch.Generator(device=ctx.device).manual_seed(5)
    genome = ctx.gen_reads(max(100_000, 20 * n), seed=0xC0FFEE)
    reads = ctx.empty(n * L, torch.uint8)
    for r0 in range(0, n, 1_000_000):                      # (in pieces: the gather's index is 8 bytes per base)
        m = min(1_000_000, n - r0)
        starts = torch.randint(0, genome.numel() - L + 1, (m,), device=ctx.device, generator=g)
        reads[r0 * L:(r0 + m) * L] = genome[(starts[:, None] + torch.arange(L, device=ctx.device)[None, :]).reshape(-1)]
    del genome
    km, cnt = ctx.count_canonical(reads, n, L, 31)
    race(ctx, "k = 31, own table", km, cnt, 31, reps)
    race(ctx, "k = 31, min_count = 2", km, cnt, 31, reps, 2)
    del km, cnt
    torch.cuda.empty_cache()
    n2 = min(n, 5_000_000)                                 # (the two-word counter's working set: 36 bytes per window)
    km, cnt = ctx.count_canonical2(reads[:n2 * L], n2, L, 47)
    race(ctx, f"k = 47, {n2:.0e} reads, own table", km, cnt, 47, reps)
    held, allocs = ctx.work_buffer_info()
    print(f"work buffer held at the end: {held / 2**30:.2f} GiB ({allocs} allocations)")
    ctx.close()


if __name__ == "__main__":
    main()
