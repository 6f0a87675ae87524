"""dev tool: kmx_count_link_support and kmx_count_adjacency_cut beside their only compositions, alternating in one process so both see
the same device state; each pair is checked equal before anything is timed.
  support composition: torch on the device -- the segment rows paired (s, s + 1), the junction and end conditions as masks, the wanted
          (t, t') and its mirror looked up by searchsorted in the sorted keys source * 2 U + target of all links, scatter_add_ of ones.
          call: count_link_support into zeroed arrays.
  cut     composition: the exit node's edge bits of every oriented unitig re-derived as in tools/bench_unitig_links.py, the slot of each
          by a cumsum along the row, the edge bytes unpacked to bits, index_put_ of zeros, packed again.
          call: count_cut_links; the mask is LinkSupport.unsupported(1) of the batch.
Both compositions are plain functions of tensors (support_composition, cut_composition), written for well-formed inputs (lists of
at most four, targets below 2 U): tests/test_link_support_np.py pins them against the host reference on the CPU.  The table is
count_canonical of the batch itself -- reads drawn from a genome at 7.5-fold coverage, 0.5 % of their bases substituted -- and the
graph and the paths are the batch's own (min_count = 1).  Beside the times it reports the links, the junctions, and the share of the
support's atomic adds that land on the 1 % of link slots that receive the most: what decides whether equal slots should be
aggregated within a wave before the atomic.  Times are wall-clock medians of synchronised calls (ms).
Output: profiles/count_link_support_bench.txt.
  python tools/bench_link_support.py [n_reads, default 1e7] [reps, default 3]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

LOW32, LOW63 = 0xFFFFFFFF, 0x7FFFFFFFFFFFFFFF


def support_composition(segments, offsets, link_offsets, targets):
    """-> (support int64[L], summary int64[3]) from the definitions of include/kmx.h, for links as kmx_count_unitig_links writes them"""
    dev = offsets.device
    n_unitigs, n_links = offsets.numel() - 1, targets.numel()
    support = torch.zeros(n_links, dtype=torch.int64, device=dev)
    if segments.shape[0] < 2:
        return support, torch.zeros(3, dtype=torch.int64, device=dev)
    a, b = segments[:-1], segments[1:]
    start, length, start2 = a[:, 1] & LOW32, (a[:, 1] >> 32) & LOW32, b[:, 1] & LOW32
    junction = (a[:, 0] == b[:, 0]) & (start2 == start + length)
    u, u2 = a[:, 2], b[:, 2]
    q, d, q2, d2 = (a[:, 3] >> 1) & LOW63, a[:, 3] & 1, (b[:, 3] >> 1) & LOW63, b[:, 3] & 1
    inside = (u >= 0) & (u < n_unitigs) & (u2 >= 0) & (u2 < n_unitigs)
    uc, u2c = u.clamp(0, max(n_unitigs - 1, 0)), u2.clamp(0, max(n_unitigs - 1, 0))
    size = (offsets[1:] - offsets[:-1]).clamp(min=0)
    if n_unitigs == 0 or n_links == 0:
        j = int(junction.sum())
        return support, torch.tensor([j, 0, j], dtype=torch.int64, device=dev)
    leaves = torch.where(d == 0, q + length == size[uc], q + 1 == length)
    enters = torch.where(d2 == 0, q2 == 0, q2 + 1 == size[u2c])
    t, t2 = 2 * uc + d, 2 * u2c + d2
    deg = link_offsets[1:] - link_offsets[:-1]
    source = torch.repeat_interleave(torch.arange(deg.numel(), device=dev), deg)
    keys, order = torch.sort(source * (2 * n_unitigs) + targets, stable=True)

    def slot_of(src, dst):
        want = src * (2 * n_unitigs) + dst
        at = torch.searchsorted(keys, want.contiguous()).clamp(max=n_links - 1)
        return keys[at] == want, order[at]

    found, slot = slot_of(t, t2)
    crossing = junction & inside & leaves & enters & found
    has_mirror, mirror = slot_of(t2 ^ 1, t ^ 1)
    support.scatter_add_(0, slot[crossing], torch.ones_like(slot[crossing]))
    twice = crossing & has_mirror & (mirror != slot)
    support.scatter_add_(0, mirror[twice], torch.ones_like(mirror[twice]))
    j, c = junction.sum(), crossing.sum()
    return support, torch.stack([j, c, j - c])


def cut_composition(edges, flips, nbr, place, nodes, offsets, link_offsets, cut):
    """-> edges_out uint8[n]; unitigs as kmx_count_unitigs(2) writes them (none empty, U >= 1), link_offsets as kmx_count_unitig_links"""
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
    ok = inside[:, None] & has & (j >= 0) & (j < n)
    x = place[torch.where(ok, j, torch.zeros_like(j))]
    p = (x >> 3) - 1
    ok &= (x != 0) & (p >= 0) & (p < n_nodes)
    same = (o[:, None] ^ f) == (x & 1)
    ok &= torch.where(same, (x & 2) != 0, (x & 4) != 0)
    slot = link_offsets[:-1, None] + torch.cumsum(ok, 1) - ok.to(torch.int64)           # the d-th link of t
    if cut.numel() == 0:
        return edges.clone()
    gone = ok & (slot < cut.numel()) & (cut[slot.clamp(0, cut.numel() - 1)] != 0)
    bits = ((edges[:, None] >> torch.arange(8, device=dev, dtype=torch.uint8)[None, :]) & 1).to(torch.bool)
    bits.index_put_((i[:, None].expand_as(e)[gone], e[gone]), torch.zeros((), dtype=torch.bool, device=dev))
    return (bits.to(torch.uint8) << torch.arange(8, device=dev, dtype=torch.uint8)[None, :]).sum(1, dtype=torch.uint8)


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
        print(f"{name:<10s} {what:<8s} MISMATCH: the call and its composition differ; not timed")
        return
    del a, b
    t = {"call": [], "comp": []}
    for _ in range(reps):
        for key, f in (("call", call), ("comp", comp)):
            ms, o = timed(f)
            t[key].append(ms)
            del o
    mc, mp = statistics.median(t["call"]), statistics.median(t["comp"])
    print(f"{name:<10s} {what:<8s} {items:>10.3e} {mc:9.3f} {items / mc / 1e6:9.3f} {mp:9.3f} {mp / mc:7.2f} {(max(t['call']) - min(t['call'])) / mc:7.2f}")


def race(ctx, name, reads, n, L, k, reps):
    km, cnt = ctx.count_canonical(reads, n, L, k)
    adj = ctx.count_adjacency(km, cnt, k, 1, flips=True, neighbors=True)
    un = ctx.count_unitigs(km, cnt, k, 1, adjacency=adj)
    n_tab = cnt.numel()
    place = ctx.count_unitig_index(un, n_tab)
    links = ctx.count_unitig_links(un, adj, n_tab, place=place)
    paths = ctx.count_read_paths(reads, n, L, k, km, un, place=place)
    sup = ctx.count_link_support(paths, un, links)
    s = sup.support
    top = torch.sort(s, descending=True).values[:max(links.n_links // 100, 1)].sum()
    print(f"{name:<10s} entries {n_tab:.3e}  unitigs {un.n_unitigs:.3e}  links {links.n_links:.3e}  segments {paths.n_segments:.3e}  junctions "
          f"{sup.junctions:.3e}  unlinked {sup.unlinked}  links without support {int((s == 0).sum()):.3e}  share of the atomic adds on the 1 % "
          f"hottest link slots {float(top) / max(float(s.sum()), 1.0):.3f}  (hottest slot: {int(s.max())})")
    _race(name, "support", lambda: ctx.count_link_support(paths, un, links),
          lambda: support_composition(paths.segments, un.offsets, links.offsets, links.targets),
          lambda a, b: torch.equal(a.support, b[0]) and torch.equal(a.summary, b[1]), reps, paths.n_segments)
    cut = sup.unsupported(1)
    _race(name, "cut", lambda: ctx.count_cut_links(un, links, adj, n_tab, cut, place=place)[0],
          lambda: cut_composition(adj[0], adj[1], adj[2], place, un.nodes, un.offsets, links.offsets, cut),
          lambda a, b: torch.equal(a, b), reps, 2 * un.n_unitigs)
    torch.cuda.empty_cache()


def main():
    from kmers_amd.api import Context

    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    ctx = Context(0)
    L = 150
    print(f"count_link_support and count_cut_links beside their torch compositions; {n:.0e} reads of {L} bp, the batch's own table, graph and "
          f"paths; median of {reps} alternating wall-clock runs each (ms); Gitems/s = items / call ms / 1e6 (support: segments, cut: oriented "
          f"unitigs); ratio = comp / call; spread = (max - min) / median of the call's runs; MI355X")
    print(f"{'batch':<10s} {'what':<8s} {'items':>10s} {'call ms':>9s} {'Gitems/s':>9s} {'comp ms':>9s} {'ratio':>7s} {'spread':>7s}")
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
    held, allocs = ctx.work_buffer_info()
    print(f"work buffer held at the end: {held / 2**30:.2f} GiB ({allocs} allocations)")
    ctx.close()


if __name__ == "__main__":
    main()
