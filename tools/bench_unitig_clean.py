"""dev tool: kmx_count_unitig_clean beside its only composition, alternating in one process so both see the same device state; the
two answers are compared before anything is timed and their agreement is printed.
  composition: torch on the device -- the Unitigs.tips mask; a padded (2U, 4) matrix of targets gathered from the link offsets; for
          the tips the targets of the side that has links, the lists of the mirrors of those targets gathered through it (U, 4, 4),
          the float64 mean counts of the siblings found there compared with the tip's own; for the bubbles the four lists that close
          one gathered and compared, then the means of the two branches.
  call:   count_unitig_clean with the links made once up front.
The composition compares float64 means where the call compares integer products.  Means that are equal as floats are taken as equal
and decided by index, as the rule decides exact ties: for the sums and lengths of a real table two unequal quotients differ by far
more than one rounding, so equal floats are equal quotients.  Means that are unequal but within 1e-12 of each other could fall either
way in floating point: such unitigs are marked as ties and left out of the comparison (their number is printed).  clean_composition
is a plain function of tensors: tests/test_clean_np.py pins it against the host reference on the CPU.
The table is count_canonical(2) of the batch itself -- reads drawn from a genome at 7.5-fold coverage, 0.5 % of their bases
substituted, so the graph has tips and bubbles -- and the unitigs are the batch's own (min_count = 1).  Times are wall-clock medians
of synchronised calls (ms).  Nothing gates on the output; it goes to profiles/count_unitig_clean_bench.txt.
  python tools/bench_unitig_clean.py [n_reads, default 1e7] [reps, default 3]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def clean_composition(unitigs, links, tip_max_nodes, tip_num, tip_den, bubble_max_nodes, bubble_max_diff, island_max_nodes):
    """-> (reason uint8[U], tie bool[U]) from the rule of include/kmx.h, for unitigs and links as the calls write them (U >= 1, none
    empty, every target < 2 U); tie[u]: a comparison of means that decided u was between two unequal floats within rounding of each other"""
    dev = unitigs.offsets.device
    U = unitigs.n_unitigs
    m = unitigs.lengths
    mean = unitigs.mean_counts
    u = torch.arange(U, device=dev)
    deg = links.degrees
    degf = deg.reshape(-1)
    c4 = torch.arange(4, device=dev)
    V = c4[None, :] < degf[:, None]
    if links.n_links:
        T = torch.where(V, links.targets[(links.offsets[:-1, None] + c4[None, :]).clamp(max=links.n_links - 1)], torch.zeros_like(V, dtype=torch.int64))
    else:
        T = torch.zeros((2 * U, 4), dtype=torch.int64, device=dev)
    linear = unitigs.circular == 0

    def lose(mu, my, iu, iy, a, b):
        l, r = mu * b, my * a
        near = torch.isclose(l, r, rtol=1e-12, atol=0.0) & (l != r)
        return (l < r) | ((l == r) & (iu > iy)), near

    reason = torch.zeros(U, dtype=torch.uint8, device=dev)
    tie = torch.zeros(U, dtype=torch.bool, device=dev)
    # islands
    if island_max_nodes > 0:
        reason[linear & (deg == 0).all(1) & (m <= island_max_nodes)] = 3
    # tips
    if tip_max_nodes > 0:
        cand = unitigs.tips(links, tip_max_nodes)
        if tip_num == 0:
            reason[cand] = 1
        else:
            t = 2 * u + (deg[:, 0] == 0).to(torch.int64)
            X, VX = T[t], V[t]
            Z, VZ = T[X ^ 1], V[X ^ 1] & VX[:, :, None]
            yu = Z >> 1
            VZ = VZ & (yu != u[:, None, None])
            lo, near = lose(mean[:, None, None], mean[yu], u[:, None, None], yu, tip_num, tip_den)
            reason[cand & (VZ & lo).any(2).any(1)] = 1
            tie |= cand & (VZ & near).any(2).any(1)
    # bubbles
    if bubble_max_nodes > 0:
        cand = linear & (deg == 1).all(1) & (m <= bubble_max_nodes)
        x, s = T[2 * u, 0], T[2 * u + 1, 0] ^ 1
        ls = T[s]
        ok = cand & (degf[s] == 2) & (ls[:, 0] != ls[:, 1]) & ((ls[:, 0] == 2 * u) | (ls[:, 1] == 2 * u))
        y = torch.where(ls[:, 1] == 2 * u, ls[:, 0], ls[:, 1])
        yu = y >> 1
        lx = T[x ^ 1]
        ok &= (degf[x ^ 1] == 2) & (((lx[:, 0] == 2 * u + 1) & (lx[:, 1] == (y ^ 1))) | ((lx[:, 0] == (y ^ 1)) & (lx[:, 1] == 2 * u + 1)))
        ok &= (degf[y] == 1) & (T[y, 0] == x) & (degf[y ^ 1] == 1) & (T[y ^ 1, 0] == (s ^ 1))
        ok &= (u != yu) & (u != s >> 1) & (u != x >> 1) & (yu != s >> 1) & (yu != x >> 1)
        ok &= linear[yu] & (m[yu] <= bubble_max_nodes) & ((m - m[yu]).abs() <= bubble_max_diff)
        lo, near = lose(mean, mean[yu], u, yu, 1, 1)
        reason[ok & lo] = 2
        tie |= ok & near
    return reason, tie


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def race(ctx, name, reads, n, L, k, reps):
    one = k <= 31
    km, cnt = (ctx.count_canonical if one else ctx.count_canonical2)(reads, n, L, k)
    adj = (ctx.count_adjacency if one else ctx.count_adjacency2)(km, cnt, k, 1, flips=True, neighbors=True)
    un = (ctx.count_unitigs if one else ctx.count_unitigs2)(km, cnt, k, 1, adjacency=adj)
    n_tab = cnt.numel()
    links = ctx.count_unitig_links(un, adj, n_tab)
    del adj
    print(f"{name:<24s} entries {n_tab:.3e}  unitigs {un.n_unitigs:.3e}  links {links.n_links:.3e}")
    rule = (k, 1, 1, 2 * k, 4, k)
    call = lambda: ctx.count_unitig_clean(un, links, island_max_nodes=k)
    comp = lambda: clean_composition(un, links, *rule)
    _, (keep, a) = timed(call)
    _, (b, tie) = timed(comp)
    c = torch.bincount(a, minlength=4).cpu().tolist()
    differ = int(((a != b) & ~tie).sum())
    print(f"{name:<24s} dropped: tips {c[1]}  bubbles {c[2]}  islands {c[3]}; left out as within rounding {int(tie.sum())}; "
          f"the call and the composition differ on {differ} of the other {un.n_unitigs - int(tie.sum())} unitigs")
    del keep, a, b, tie
    t = {"call": [], "comp": []}
    for _ in range(reps):
        for key, f in (("call", call), ("comp", comp)):
            ms, o = timed(f)
            t[key].append(ms)
            del o
    mc, mp = statistics.median(t["call"]), statistics.median(t["comp"])
    items = un.n_unitigs
    print(f"{name:<24s} {'clean':<7s} {items:>10.3e} {mc:9.3f} {items / mc / 1e6:9.3f} {mp:9.3f} {mp / mc:6.2f} {(max(t['call']) - min(t['call'])) / mc:7.2f}")
    torch.cuda.empty_cache()


def main():
    from kmers_amd.api import Context

    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    ctx = Context(0)
    L = 150
    print(f"count_unitig_clean (tips of at most k nodes at ratio 1/1, bubbles of at most 2 k, islands of at most k) beside its torch composition; {n:.0e} reads of {L} bp, the batch's "
          f"own table, unitigs and links; median of {reps} alternating wall-clock runs each (ms); Gitems/s = unitigs / call ms / 1e6; "
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
    ctx.close()


if __name__ == "__main__":
    main()
