"""dev tool: kmx_count_unitig_links and kmx_count_unitig_select(2) beside their only compositions, alternating in one process so both
see the same device state; each pair is checked equal before anything is timed.
  links   composition: torch on the device -- the exit node of every oriented unitig gathered from the node list, its edge and flip
          byte, the four neighbour words of its side and their places gathered, searchsorted for the unitig of every place, a
          cumsum of the degrees for the offsets, a boolean index (nonzero) for the targets.
          call: count_unitig_links with the index made once up front and room for the links known (one call, no counting pass).
  select  composition: place -> searchsorted -> keep[...] -> nonzero -> gathers of keys and counts.
          call: count_unitig_select(2) with the same index; the keep mask drops a random tenth of the unitigs.
Both compositions are plain functions of tensors (links_composition, select_composition): tests/test_link_np.py pins them against
the host reference on the CPU.  The table is count_canonical(2) of the batch itself -- reads drawn from a genome at 7.5-fold
coverage, 0.5 % of their bases substituted, so the graph has tips and bubbles -- and the unitigs are the batch's own (min_count = 1).
Times are wall-clock medians of synchronised calls (ms).  Output: profiles/count_unitig_links_bench.txt.
  python tools/bench_unitig_links.py [n_reads, default 1e7] [reps, default 3]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def links_composition(edges, flips, nbr, place, nodes, offsets):
    """-> (link offsets int64[2U + 1], targets int64[L]) from the definitions of include/kmx.h; unitigs as kmx_count_unitigs(2)
    writes them (none empty, U >= 1), any bytes in the other arrays"""
    dev = offsets.device
    n, n_nodes = edges.numel(), offsets[-1]
    v = torch.stack([nodes[offsets[1:] - 1], nodes[offsets[:-1]] ^ 1], 1).reshape(-1)   # the exit node of t = 2 u + s
    i, o = v >> 1, v & 1
    inside = (i >= 0) & (i < n)
    i = torch.where(inside, i, torch.zeros_like(i))
    e = 4 * o[:, None] + torch.arange(4, device=dev)[None, :]
    has = ((edges[i].to(torch.int64)[:, None] >> e) & 1) != 0
    f = (flips[i].to(torch.int64)[:, None] >> e) & 1
    j = nbr.reshape(-1, 8)[i[:, None], e]
    ok = inside[:, None] & has & (j >= 0) & (j < n)                                      # (a u64 at or above 2^63 reads negative)
    x = place[torch.where(ok, j, torch.zeros_like(j))]
    p = (x >> 3) - 1
    ok &= (x != 0) & (p >= 0) & (p < n_nodes)
    same = (o[:, None] ^ f) == (x & 1)
    ok &= torch.where(same, (x & 2) != 0, (x & 4) != 0)
    u2 = torch.searchsorted(offsets, p.clamp(min=0).contiguous(), right=True) - 1
    link_offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(ok.sum(1), 0)])
    return link_offsets, (2 * u2 + (~same).to(torch.int64))[ok]


def select_mask(place, offsets, keep):
    """bool[n]: the entry lies in a kept unitig (U >= 1)"""
    p = (place >> 3) - 1
    ok = (place != 0) & (p >= 0) & (p < offsets[-1])
    u = (torch.searchsorted(offsets, p.clamp(min=0).contiguous(), right=True) - 1).clamp(max=keep.numel() - 1)
    return ok & (keep[u] != 0)


def select_composition(kmers, counts, place, offsets, keep):
    """-> (kmers, counts) of the entries in kept unitigs (U >= 1)"""
    idx = torch.nonzero(select_mask(place, offsets, keep))[:, 0]
    if kmers.dim() == 1:
        return kmers[idx], counts[idx]
    # (two-word keys: one-dimensional gathers of the two words.  In one run at n = 2.6e8, kmers[mask] on the (n, 2) tensor gave
    # rows of zeros where the call gave keys; that is not yet explained, this form does not depend on it, and race() prints
    # whether the two forms agree)
    flat = kmers.reshape(-1)
    return torch.stack([flat[2 * idx], flat[2 * idx + 1]], 1), counts[idx]


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _race(name, what, call, comp, equal, reps, items):
    _, a = timed(call)
    _, b = timed(comp)
    if not equal(a, b):
        print(f"{name:<24s} {what:<7s} MISMATCH: the call and its composition differ; not timed")
        return
    del a, b
    t = {"call": [], "comp": []}
    for _ in range(reps):
        for key, f in (("call", call), ("comp", comp)):
            ms, o = timed(f)
            t[key].append(ms)
            del o
    mc, mp = statistics.median(t["call"]), statistics.median(t["comp"])
    print(f"{name:<24s} {what:<7s} {items:>10.3e} {mc:9.3f} {items / mc / 1e6:9.3f} {mp:9.3f} {mp / mc:6.2f} {(max(t['call']) - min(t['call'])) / mc:7.2f}")


def race(ctx, name, reads, n, L, k, reps):
    one = k <= 31
    km, cnt = (ctx.count_canonical if one else ctx.count_canonical2)(reads, n, L, k)
    adj = (ctx.count_adjacency if one else ctx.count_adjacency2)(km, cnt, k, 1, flips=True, neighbors=True)
    un = (ctx.count_unitigs if one else ctx.count_unitigs2)(km, cnt, k, 1, adjacency=adj)
    n_tab = cnt.numel()
    place = ctx.count_unitig_index(un, n_tab)
    links = ctx.count_unitig_links(un, adj, n_tab, place=place)
    print(f"{name:<24s} entries {n_tab:.3e}  unitigs {un.n_unitigs:.3e}  links {links.n_links:.3e}")
    L_ = links.n_links
    _race(name, "links", lambda: ctx.count_unitig_links(un, adj, n_tab, place=place, max_links=L_),
          lambda: links_composition(adj[0], adj[1], adj[2], place, un.nodes, un.offsets),
          lambda a, b: torch.equal(a.offsets, b[0]) and torch.equal(a.targets, b[1]), reps, 2 * un.n_unitigs)
    del links
    g = torch.Generator(device=ctx.device).manual_seed(7)
    keep = (torch.rand(un.n_unitigs, device=ctx.device, generator=g) >= 0.1).to(torch.uint8)
    sel = ctx.count_unitig_select if one else ctx.count_unitig_select2
    _race(name, "select", lambda: sel(km, cnt, un, keep, place=place), lambda: select_composition(km, cnt, place, un.offsets, keep),
          lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), reps, n_tab)
    if not one:
        same = torch.equal(km[select_mask(place, un.offsets, keep)], select_composition(km, cnt, place, un.offsets, keep)[0])
        print(f"{name:<24s} kmers[mask] on the (n, 2) key tensor equals the one-dimensional gathers of the composition: {same}")
    torch.cuda.empty_cache()


def main():
    from kmers_amd.api import Context

    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    ctx = Context(0)
    L = 150
    print(f"count_unitig_links and count_unitig_select(2) beside their torch compositions; {n:.0e} reads of {L} bp, the batch's own table and "
          f"unitigs; median of {reps} alternating wall-clock runs each (ms); Gitems/s = items / call ms / 1e6 (links: oriented unitigs, select: entries); "
          f"ratio = comp / call; spread = (max - min) / median of the call's runs; MI355X")
    print(f"{'batch':<24s} {'what':<7s} {'items':>10s} {'call ms':>9s} {'Gitems/s':>9s} {'comp ms':>9s} {'ratio':>6s} {'spread':>7s}")
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
