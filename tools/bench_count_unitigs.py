"""dev tool: kmx_count_unitigs(2) beside its only composition, alternating in one process so both see the same device state; the two
are checked equal before anything is timed.
  composition  the same links and the same pointer jumping written in torch on the device -- one gather per field and round over all
               oriented nodes, a host read of the stop counters per round -- then compaction by torch cumsum and scatter.
  call         count_unitigs(2) on the adjacency made once up front (edges, flips, neighbour indices), all outputs.
The table is count_canonical(2) of reads drawn from a genome at 7.5-fold coverage.  Times are wall-clock medians of synchronised
calls (ms).  Rounds are those of the composition (the call runs the same recurrence); bytes per round follow DESIGN 4.6.6: 32 bytes
streamed per oriented node and 16 gathered per node still open at the start of the round.  Output: profiles/count_unitigs_bench.txt.
  python tools/bench_count_unitigs.py [n_reads, default 1e7] [reps, default 3]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from kmers_amd.api import Context

POP = [bin(v).count("1") for v in range(16)]
LOW = [(v & -v).bit_length() - 1 if v else 0 for v in range(16)]


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def composition(edges, flips, nbr, counts, min_count, pal=None, stats=None):
    """-> nodes, offsets, circular, count_sums (int64 tensors), from the definitions of include/kmx.h"""
    dev = edges.device
    n = edges.numel()
    pop, low = torch.tensor(POP, device=dev), torch.tensor(LOW, device=dev)
    i = torch.arange(n, device=dev)
    present = torch.ones(n, dtype=torch.bool, device=dev) if counts is None else counts >= min_count
    e64, f64 = edges.to(torch.int64), flips.to(torch.int64)
    cand = torch.full((2 * n,), -1, dtype=torch.int64, device=dev)
    for o in (0, 1):
        nib = (e64 >> (4 * o)) & 15
        e = 4 * o + low[nib]
        j = nbr.view(n, 8).gather(1, e[:, None])[:, 0]
        ok = present & (pop[nib] == 1) & (j >= 0) & (j < n) & (j != i)
        js = torch.where(ok, j, 0)
        f = (f64 >> e) & 1
        other = e64[js]
        ok &= pop[torch.where((o ^ f) == 0, other >> 4, other & 15)] == 1
        if pal is not None:
            ok &= ~pal & ~pal[js]
        cand[o::2] = torch.where(ok, 2 * js + (o ^ f), -1)
    v = torch.arange(2 * n, device=dev)
    nxt = torch.where((cand >= 0) & (cand[cand.clamp(min=0) ^ 1] == (v ^ 1)), cand, -1)
    w = nxt[v ^ 1]
    prev = torch.where(w >= 0, w ^ 1, -1)
    del cand, nxt, w
    done = prev < 0
    ptr, val, mn = torch.where(done, v, prev), torch.zeros_like(v), v.clone()
    n_open, rounds, gathered = int((~done).sum()), 0, []
    while n_open:
        d = 1 << rounds
        gathered.append(n_open)
        act = ~done
        q_done, q_ptr, q_val, q_mn = done[ptr], ptr[ptr], val[ptr], mn[ptr]
        fin = act & q_done
        upd = act & ~q_done & (q_mn < mn)
        val = torch.where(fin | upd, d + q_val, val)
        mn = torch.where(upd, q_mn, mn)
        ptr = torch.where(act, q_ptr, ptr)
        done = done | fin
        rounds += 1
        n_fin, n_upd = int(fin.sum()), int(upd.sum())
        n_open -= n_fin
        if n_fin == 0 and n_upd == 0:
            break
    head = torch.where(done, ptr, mn)
    ent, o = v >> 1, v & 1
    tail_ent = head[v ^ 1] >> 1
    chain = done & (ptr == v) & present[ent] & ((ent < tail_ent) | ((ent == tail_ent) & (o == 0)))
    cycle = ~done & (mn == v) & (o == 0)
    length = torch.where(chain, val[v ^ 1] + 1, torch.where(cycle, val[prev.clamp(min=0)] + 1, 0))
    heads = torch.nonzero(chain | cycle)[:, 0]
    lens = length[heads]
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    uid_of = torch.full((2 * n,), -1, dtype=torch.int64, device=dev)
    uid_of[heads] = torch.arange(heads.numel(), device=dev)
    uid = uid_of[head]
    sel = torch.nonzero(uid >= 0)[:, 0]
    nodes = torch.empty(int(offsets[-1]), dtype=torch.int64, device=dev)
    nodes[offsets[uid[sel]] + val[sel]] = sel
    sums = torch.zeros(heads.numel(), dtype=torch.int64, device=dev)
    sums.index_add_(0, uid[sel], torch.ones_like(sel) if counts is None else counts[sel >> 1])
    if stats is not None:
        stats.update(rounds=rounds, gathered=gathered, longest=int(lens.max()) if lens.numel() else 0, n_nodes=2 * n)
    return nodes, offsets, cycle[heads].to(torch.uint8), sums


def race(ctx, name, km, cnt, k, reps, min_count=1):
    one = k <= 31
    adj = (ctx.count_adjacency if one else ctx.count_adjacency2)(km, cnt, k, min_count, flips=True, neighbors=True)
    uni = ctx.count_unitigs if one else ctx.count_unitigs2
    n = cnt.numel()
    call = lambda: uni(km, cnt, k, min_count, adjacency=adj)
    stats = {}
    comp = lambda: composition(adj[0], adj[1], adj[2], cnt, min_count, None, stats)   # (odd k: no palindromes)
    _, a = timed(call)
    _, b = timed(comp)
    same = (torch.equal(a.nodes, b[0]) and torch.equal(a.offsets, b[1]) and torch.equal(a.circular, b[2]) and torch.equal(a.count_sums, b[3]))
    if not same:
        print(f"{name:<34s} MISMATCH: the call and its composition differ; not timed")
        return
    n_unitigs = a.n_unitigs
    del a, b
    t = {"call": [], "comp": []}
    for _ in range(reps):
        for key, f in (("call", call), ("comp", comp)):
            ms, o = timed(f)
            t[key].append(ms)
            del o
    mc, mp = statistics.median(t["call"]), statistics.median(t["comp"])
    spread = (max(t["call"]) - min(t["call"])) / mc
    r = stats["rounds"]
    model = [32 * stats["n_nodes"] + 16 * g for g in stats["gathered"]]
    print(f"{name:<34s} {n:>10.3e} {n_unitigs:>10.3e} {stats['longest']:>8d} {r:>6d} {mc:9.2f} {mc / max(r, 1):9.2f} {mp:9.2f} {mp / mc:6.2f} {spread:7.2f}   "
          f"model GB/round first {model[0] / 1e9:.2f} last {model[-1] / 1e9:.2f}, gathered nodes/round {stats['gathered']}")
    torch.cuda.empty_cache()


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    ctx = Context(0)
    L = 150
    print(f"count_unitigs(2) beside the same pointer jumping in torch gathers and compaction by torch scan and scatter; tables of {n:.0e} reads of "
          f"{L} bp; median of {reps} alternating wall-clock runs each (ms); ms/round = call ms / rounds (links and compaction included); ratio = "
          f"comp / call; spread = (max - min) / median of the call's runs; MI355X")
    print(f"{'table':<34s} {'entries':>10s} {'unitigs':>10s} {'longest':>8s} {'rounds':>6s} {'call ms':>9s} {'ms/round':>9s} {'comp ms':>9s} {'ratio':>6s} {'spread':>7s}")
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
