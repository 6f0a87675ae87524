"""dev tool: the two reductions over a coloured table beside what a caller had before them, alternating in one process so both see the
same device state.
  count_read_colors   against count_lookup_reads with the masks as the counts (8 bytes per window), the windows' flags, and torch
                      bit reductions over the (reads, windows) array of masks -- unpacked to one byte per (window, colour), a chunk
                      of reads at a time -- for the rows and the hit counts;
  count_color_matrix  against the torch composition on the same table: the masks unpacked to a (keys, colours) matrix B of float64
                      (exact below 2^53), B.T @ B, and a bincount of the row sums for the spectrum.
The table: n_colors samples, each the k-mers of a stretch of half a random genome, the stretches evenly staggered, folded with
count_color_build; the reads are cut from the genome at random.  Both sides are checked equal -- every word of the rows, the hit
counts, the matrix and the spectrum -- before anything is timed; MISMATCH is printed otherwise.  Times are wall-clock medians of
synchronised calls (ms).  Output: profiles/colors_bench.txt.
  python tools/bench_colors.py [n_reads, default 1e6] [reps, default 3]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from kmers_amd.api import Context

CHUNK = 20_000   # reads per step of the composition: 20 000 * 120 windows * 64 colours bytes of unpacked bits


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def pack(flags, shifts):
    """(n, n_colors) bool -> int64 masks (distinct bits: the sum is the OR; bit 63 wraps into the sign, as it should)"""
    return (flags.long() << shifts).sum(1)


def rows_composition(ctx, bases, n, L, k, km, colors, nc, thr):
    dev = ctx.device
    W = L - k + 1
    masks = ctx.count_lookup_reads(bases, n, L, k, km, colors).view(n, W)
    valid = (ctx.canonical_windows(bases, n, L, k, want=("flags",))["flags"].view(n, W) & 1).bool()
    if nc < 64:
        masks = masks & ((1 << nc) - 1)
    masks = torch.where(valid, masks, torch.zeros_like(masks))
    shifts = torch.arange(nc, device=dev)
    rows = torch.empty((n, 8), dtype=torch.int64, device=dev)
    hits_out = torch.empty((n, nc), dtype=torch.int32, device=dev)
    for r0 in range(0, n, CHUNK):
        m = masks[r0:r0 + CHUNK]
        hit = m != 0
        n_valid, n_hit = valid[r0:r0 + CHUNK].sum(1), hit.sum(1)
        bits = ((m[:, :, None] >> shifts) & 1).to(torch.uint8)
        hits = bits.sum(1, dtype=torch.int64)
        some = hits > 0
        best = (hits * 64 + (63 - shifts)).max(1).values
        out = rows[r0:r0 + CHUNK]
        out[:, 0], out[:, 1] = n_valid, n_hit
        out[:, 2] = (hit & ((m & (m - 1)) == 0)).sum(1)
        out[:, 3] = pack(some & (hits == n_hit[:, None]), shifts)
        out[:, 4] = pack(some, shifts)
        out[:, 5] = pack(some & (hits * thr[1] >= thr[0] * n_valid[:, None]), shifts)
        out[:, 6] = torch.where(n_hit > 0, ((best // 64) << 32) | (63 - best % 64), torch.zeros_like(best))
        out[:, 7] = (hit[:, :-1] & hit[:, 1:] & (m[:, :-1] != m[:, 1:])).sum(1)
        hits_out[r0:r0 + CHUNK] = hits.to(torch.int32)
    return rows, hits_out


def matrix_composition(colors, nc):
    shifts = torch.arange(nc, device=colors.device)
    B = ((colors[:, None] >> shifts) & 1).to(torch.float64)
    return (B.T @ B).long(), torch.bincount(B.sum(1).long(), minlength=nc + 1)


def race(name, size, call, comp, same, reps):
    """check equal, then alternate the two; prints one row"""
    _, got = timed(call)
    _, ref = timed(comp)
    ok = same(got, ref)
    del got, ref
    if not ok:
        print(f"{name:<52s} MISMATCH: the call and its composition differ; not timed")
        return
    t = {"call": [], "comp": []}
    for _ in range(reps):
        for key, f in (("call", call), ("comp", comp)):
            ms, o = timed(f)
            t[key].append(ms)
            del o
    mc, mp = statistics.median(t["call"]), statistics.median(t["comp"])
    print(f"{name:<52s} {size:>10.3e} {mc:9.3f} {mp:9.2f} {mp / mc:7.1f} {(max(t['call']) - min(t['call'])) / mc:7.2f}")
    torch.cuda.empty_cache()


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    ctx = Context(0)
    L, k, thr = 150, 31, (1, 2)
    print(f"count_read_colors and count_color_matrix beside their torch compositions; {n:.0e} reads of {L} bp, k = {k}, threshold {thr[0]}/{thr[1]}; "
          f"median of {reps} alternating wall-clock runs each (ms); spread = (max - min) / median of the call's runs; MI355X")
    print(f"{'shape':<52s} {'size':>10s} {'call ms':>9s} {'comp ms':>9s} {'ratio':>7s} {'spread':>7s}")
    g = torch.Generator(device=ctx.device).manual_seed(7)
    G = 3_000_000
    genome = ctx.gen_reads(G, seed=0xC0105)
    reads = ctx.empty(n * L, torch.uint8)
    for r0 in range(0, n, 1_000_000):                             # (in pieces: the gather's index is 8 bytes per base)
        m = min(1_000_000, n - r0)
        starts = torch.randint(0, G - L + 1, (m,), device=ctx.device, generator=g)
        reads[r0 * L:(r0 + m) * L] = genome[(starts[:, None] + torch.arange(L, device=ctx.device)[None, :]).reshape(-1)]
    for nc in (8, 64):
        per = (G // 2) // L                                        # a sample: half the genome as reads laid end to end
        tables = []
        for i in range(nc):
            a = (i * (G // 2)) // nc
            tables.append(ctx.count_canonical(genome[a:a + per * L], per, L, k))
        table = ctx.count_color_build(tables, k=k)
        del tables
        km, colors, n_keys = table.kmers, table.colors, int(table.colors.numel())
        rows = ctx.empty(8 * n, torch.int64)
        race(f"count_read_colors, {nc} colours, {n_keys:.2e} keys, hits", n * (L - k + 1),
             lambda: ctx.count_read_colors(reads, n, L, k, km, colors, nc, threshold=thr, hits=True, out=rows),
             lambda: rows_composition(ctx, reads, n, L, k, km, colors, nc, thr),
             lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), reps)
        race(f"count_color_matrix, {nc} colours", n_keys, lambda: ctx.count_color_matrix(colors, nc),
             lambda: matrix_composition(colors, nc),
             lambda a, b: torch.equal(a.shared, b[0]) and torch.equal(a.spectrum, b[1]), reps)
        del table, km, colors
        torch.cuda.empty_cache()
    held, allocs = ctx.work_buffer_info()
    print(f"work buffer held at the end: {held / 2**30:.2f} GiB ({allocs} allocations)")
    ctx.close()


if __name__ == "__main__":
    main()
