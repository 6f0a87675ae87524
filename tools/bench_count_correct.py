"""dev tool: kmx_count_correct_reads(2) beside kmx_count_read_stats(2) on the same input -- the same front half (windows call, lookup),
so the difference is what the decision costs -- and, for uniform reads at k <= 31, beside a torch composition of the rule; alternating
in one process so all see the same device state.  The composition: count_lookup_reads and the windows' flags, the candidate mask from
the unfolded valid / solid arrays, then for each of the three other bases the windows that cover a candidate spelled as bytes with
the base in place, through kmers_from_bytes, canonical_words and count_lookup.  The call and the composition are checked equal byte
for byte before anything is timed; MISMATCH is printed otherwise.  Times are wall-clock medians of synchronised calls (ms).
Output: profiles/count_correct_bench.txt.
  python tools/bench_count_correct.py [n_reads, default 1e6] [reps, default 3]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from kmers_amd.api import Context


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def composition(ctx, bases, n, L, k, km, cnt, sm, mc):
    """the corrected bytes of uniform reads, k <= 31, from calls a caller had before: the rule of kmx.h, vectorised"""
    dev = ctx.device
    W = L - k + 1
    c = ctx.count_lookup_reads(bases, n, L, k, km, cnt).view(n, W)
    valid = (ctx.canonical_windows(bases, n, L, k, want=("flags",))["flags"].view(n, W) & 1).bool()
    solid = valid & (c >= sm)
    pad = torch.nn.functional.pad
    cover = pad(valid, (k - 1, k - 1)).unfold(1, k, 1)                 # (n, L, k): [r, p, j] = valid(window p - k + 1 + j)
    n_cover = cover.sum(2)
    any_solid = pad(solid, (k - 1, k - 1)).unfold(1, k, 1).any(2)
    lut = torch.full((256,), 4, dtype=torch.int64, device=dev)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = lut[ch | 0x20] = i
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    b = bases.view(n, L)
    code = lut[b.long()]
    cand = (code < 4) & (n_cover >= mc) & ~any_solid
    r, p = torch.nonzero(cand, as_tuple=True)
    out = bases.clone()
    n_cand = r.numel()
    if n_cand == 0:
        return out
    j = torch.arange(k, device=dev)
    ci, jj = torch.nonzero(cover[r, p], as_tuple=True)                   # the valid windows that cover each candidate
    w = p[ci] - (k - 1) + jj
    at = p[ci] - w                                                       # the base's place in its window
    seqs = b.reshape(-1)[(r[ci] * L + w)[:, None] + j[None, :]]          # (M, k) bytes, all valid
    rows = torch.arange(seqs.shape[0], device=dev)
    fixes = torch.zeros((n_cand, 3), dtype=torch.bool, device=dev)
    for step in (1, 2, 3):
        alt = (code[r, p] + step) % 4
        s = seqs.clone()
        s[rows, at] = letters[alt[ci]]
        words = ctx.kmers_from_bytes(s.reshape(-1), s.shape[0], k)
        canon, _ = ctx.canonical_words(words, k)
        below = ctx.count_lookup(km, cnt, k, canon) < sm
        n_below = torch.zeros(n_cand, dtype=torch.int64, device=dev).index_add_(0, ci, below.long())
        fixes[:, step - 1] = n_below == 0
    one = fixes.sum(1) == 1
    alt = (code[r, p] + fixes.long().argmax(1) + 1) % 4
    flat = (r * L + p)[one]
    out[flat] = letters[alt[one]] | (bases[flat] & 0x20)
    return out


def race(name, call, stats, comp, reps, n_win):
    """check equal, then alternate the three; prints one row"""
    _, (got, rows) = timed(call)
    changed = int((rows.view(-1, 4)[:, 2]).sum().item())
    if comp is not None:
        _, ref = timed(comp)
        same = torch.equal(got, ref)
        del ref
        if not same:
            print(f"{name:<46s} MISMATCH: the call and its composition differ; not timed")
            return
    del got, rows
    t = {"call": [], "stats": [], "comp": []}
    for _ in range(reps):
        for key, f in (("call", call), ("stats", stats), ("comp", comp)):
            if f is not None:
                ms, o = timed(f)
                t[key].append(ms)
                del o
    mc, ms_ = statistics.median(t["call"]), statistics.median(t["stats"])
    spread = (max(t["call"]) - min(t["call"])) / mc
    if comp is not None:
        mp = statistics.median(t["comp"])
        tail = f"{mp:9.2f} {mp / mc:6.2f}"
    else:
        tail = f"{'-':>9s} {'-':>6s}"
    print(f"{name:<46s} {n_win:>10.3e} {changed:>9d} {mc:9.2f} {ms_:9.2f} {mc - ms_:9.2f} {(mc - ms_) * 1e6 / n_win:8.4f} {tail} {spread:7.2f}")
    torch.cuda.empty_cache()


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    ctx = Context(0)
    L, sm, mc = 150, 3, 1
    print(f"count_correct_reads(2) beside count_read_stats(2) and the torch composition of the rule; {n:.0e} reads, solid_min = {sm}, "
          f"min_cover = {mc}; median of {reps} alternating wall-clock runs each (ms); decide = call - stats; spread = (max - min) / median "
          f"of the call's runs; MI355X")
    print(f"{'shape':<46s} {'windows':>10s} {'corrected':>9s} {'call ms':>9s} {'stats ms':>9s} {'decide ms':>9s} {'ns/win':>8s} {'comp ms':>9s} "
          f"{'ratio':>6s} {'spread':>7s}")
    g = torch.Generator(device=ctx.device).manual_seed(5)
    genome = ctx.gen_reads(max(100_000, 5 * n), seed=0xC0FFEE)           # 30-fold coverage at 150 bp

    def draw(nr, Lr, err):
        reads = ctx.empty(nr * Lr, torch.uint8)
        for r0 in range(0, nr, 1_000_000):                             # (in pieces: the gather's index is 8 bytes per base)
            m = min(1_000_000, nr - r0)
            starts = torch.randint(0, genome.numel() - Lr + 1, (m,), device=ctx.device, generator=g)
            reads[r0 * Lr:(r0 + m) * Lr] = genome[(starts[:, None] + torch.arange(Lr, device=ctx.device)[None, :]).reshape(-1)]
        if err:
            hit = torch.nonzero(torch.rand(nr * Lr, device=ctx.device, generator=g) < err).flatten()
            swap = torch.tensor(list(b"CGTA"), dtype=torch.uint8, device=ctx.device)       # A -> C -> G -> T -> A
            lut = torch.zeros(256, dtype=torch.int64, device=ctx.device)
            for i, ch in enumerate(b"ACGT"):
                lut[ch] = i
            reads[hit] = swap[lut[reads[hit].long()]]
        return reads

    def row(tag, k, bases, nr, Lr, table, with_comp):
        one = k <= 31
        km, cnt = table
        fix = ctx.count_correct_reads if one else ctx.count_correct_reads2
        stats = ctx.count_read_stats if one else ctx.count_read_stats2
        out = ctx.empty(nr * Lr, torch.uint8)
        st = ctx.empty(8 * nr, torch.int64)
        call = lambda: fix(bases, nr, Lr, k, km, cnt, solid_min=sm, min_cover=mc, out=out)
        comp = (lambda: composition(ctx, bases, nr, Lr, k, km, cnt, sm, mc)) if with_comp and one else None
        race(tag, call, lambda: stats(bases, nr, Lr, k, km, cnt, solid_min=sm, out=st), comp, reps, nr * (Lr - k + 1))

    clean = draw(n, L, 0.0)
    noisy = draw(n, L, 0.01)
    table = ctx.count_canonical(noisy, n, L, 31)
    row("150 bp, k = 31, clean reads", 31, clean, n, L, table, True)
    row("150 bp, k = 31, 1 % substitutions, own table", 31, noisy, n, L, table, True)
    other = ctx.gen_reads(n * L, seed=0xFACE)
    row("150 bp, k = 31, reads weak throughout", 31, other, n, L, table, min(n, 100_000) == n)
    nw = min(n, 20_000)
    row(f"150 bp, k = 31, {nw:.0e} reads weak throughout", 31, other[:nw * L], nw, L, table, True)
    del other, table
    torch.cuda.empty_cache()
    table15 = ctx.count_canonical(noisy, n, L, 15)
    row("150 bp, k = 15, 1 % substitutions, own table", 15, noisy, n, L, table15, True)
    del table15
    table2 = ctx.count_canonical2(noisy, n, L, 47)
    row("150 bp, k = 47, 1 % substitutions, own table", 47, noisy, n, L, table2, False)
    del table2
    torch.cuda.empty_cache()
    # ragged reads: the same bytes cut at other places
    rng = np.random.default_rng(12)
    lens = rng.integers(100, 161, n).astype(np.uint64)
    keep = np.cumsum(lens) <= n * L
    lens = lens[keep]
    h_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    d_off = ctx.to_device(h_off)
    nr = len(lens)
    table = ctx.count_canonical(noisy, nr, 160, 31, offsets=d_off)
    out = ctx.empty(n * L, torch.uint8)
    st = ctx.empty(8 * nr, torch.int64)
    n_win = int(np.maximum(lens.astype(np.int64) - 30, 0).sum())
    race("100-160 bp ragged, k = 31, 1 % substitutions", lambda: ctx.count_correct_reads(noisy, nr, 160, 31, *table, solid_min=sm, min_cover=mc, offsets=d_off, out=out),
         lambda: ctx.count_read_stats(noisy, nr, 160, 31, *table, solid_min=sm, offsets=d_off, out=st), None, reps, n_win)
    held, allocs = ctx.work_buffer_info()
    print(f"work buffer held at the end: {held / 2**30:.2f} GiB ({allocs} allocations)")
    ctx.close()


if __name__ == "__main__":
    main()
