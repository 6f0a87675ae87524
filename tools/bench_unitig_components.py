"""dev tool: kmx_count_unitig_components beside its only composition, alternating in one process so both see the same device state;
the two answers are compared on every word before anything is timed.
  composition: torch on the device -- the edge list (links.sources() >> 1, links.targets >> 1), self-links dropped; rounds of two
          scatter_reduce_(amin) over it (every unitig takes the smallest label among its neighbours', both directions) and one gather
          (label = label[label], the shortcut) until a round changes nothing; unique(return_inverse) of the labels for the roots and
          the ids; three scatter_add_ for the records.
  call:   count_unitig_components with the links made once up front, labels, ids and records (stats=True is two calls: it counts the
          components, then allocates; the tool times ONE call with room for the records known, as bench_unitig_links.py does).
components_composition is a plain function of tensors: tests/test_component_np.py pins it against the host reference on the CPU.
The table is count_canonical of the batch itself -- reads drawn from a genome at 7.5-fold coverage, 0.5 % of their bases
substituted -- and the unitigs are the batch's own (min_count = 1): the stretches of the genome between two gaps in the coverage,
each a long chain of unitigs with bubbles and tips on it, numbered by their head entries and so in no order along it -- what a
schedule has to double its way through.  Times are wall-clock medians of synchronised calls (ms).  Nothing gates on the output; it
goes to profiles/unitig_components_bench.txt.
  python tools/bench_unitig_components.py [n_reads, default 1e7] [reps, default 3]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def components_composition(unitigs, links, mask=None):
    """-> (labels int64[U], ids int64[U], records int64[C, 4], rounds) from the rule of include/kmx.h, for unitigs and links as the
    calls write them (at most four links per side, every target < 2 U); mask: bool[U] or None; -1 where a unitig is not alive"""
    dev = links.offsets.device
    U = unitigs.n_unitigs
    a, b = links.sources() >> 1, links.targets >> 1
    ok = a != b
    if mask is not None:
        ok &= mask[a] & mask[b]
    a, b = a[ok], b[ok]
    lab = torch.arange(U, device=dev)
    rounds = 0
    while True:
        rounds += 1
        new = lab.clone()
        new.scatter_reduce_(0, a, lab[b], "amin")
        new.scatter_reduce_(0, b, lab[a], "amin")
        new = new[new]
        if torch.equal(new, lab):
            break
        lab = new
    alive = torch.ones(U, dtype=torch.bool, device=dev) if mask is None else mask
    roots, inverse = torch.unique(lab[alive], return_inverse=True)
    labels = torch.full((U,), -1, dtype=torch.int64, device=dev)
    ids = labels.clone()
    labels[alive], ids[alive] = lab[alive], inverse
    rec = torch.zeros((roots.numel(), 4), dtype=torch.int64, device=dev)
    rec[:, 0] = roots
    m = unitigs.lengths
    for col, w in ((1, torch.ones_like(m)), (2, m), (3, m if unitigs.count_sums is None else unitigs.count_sums)):
        rec[:, col].scatter_add_(0, inverse, w[alive])
    return labels, ids, rec, rounds


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def race(ctx, name, reads, n, L, k, reps):
    from kmers_amd.api import _ptr

    km, cnt = ctx.count_canonical(reads, n, L, k)
    adj = ctx.count_adjacency(km, cnt, k, 1, flips=True, neighbors=True)
    un = ctx.count_unitigs(km, cnt, k, 1, adjacency=adj)
    n_tab = cnt.numel()
    links = ctx.count_unitig_links(un, adj, n_tab)
    del adj
    U = un.n_unitigs
    print(f"{name:<24s} entries {n_tab:.3e}  unitigs {U:.3e}  links {links.n_links:.3e}")
    first = ctx.count_unitig_components(un, links)
    n_comp = first.n_components
    labels, ids, rec = ctx.empty(U, torch.int64), ctx.empty(U, torch.int64), ctx.empty(4 * n_comp, torch.int64)

    def call():
        c, r = C.c_uint64(0), C.c_uint32(0)
        with torch.cuda.stream(ctx.stream):
            ctx._ck(ctx.lib.kmx_count_unitig_components(ctx._h, _ptr(un.offsets), _ptr(un.count_sums), U, _ptr(links.offsets), _ptr(links.targets),
                                                        links.n_links, None, _ptr(labels), _ptr(ids), _ptr(rec), n_comp, C.byref(c), C.byref(r)))
        return int(c.value), int(r.value)

    comp = lambda: components_composition(un, links)
    _, (c_call, rounds) = timed(call)
    _, (b_labels, b_ids, b_rec, b_rounds) = timed(comp)
    assert c_call == n_comp == b_rec.shape[0]
    assert torch.equal(labels, b_labels) and torch.equal(ids, b_ids) and torch.equal(rec.view(-1, 4), b_rec)   # every word
    assert torch.equal(first.labels, labels) and torch.equal(first.records, rec.view(-1, 4))
    sizes = b_rec[:, 1]
    print(f"{name:<24s} components {n_comp:.3e}: the largest holds {int(sizes.max())} unitigs and {int(b_rec[:, 2].max())} nodes, {int((sizes == 1).sum())} "
          f"are single unitigs; rounds: the call {rounds}, the composition {b_rounds}; the call and the composition agree on every word")
    del b_labels, b_ids, b_rec, first
    t = {"call": [], "comp": []}
    for _ in range(reps):
        for key, f in (("call", call), ("comp", comp)):
            ms, o = timed(f)
            t[key].append(ms)
            del o
    mc, mp = statistics.median(t["call"]), statistics.median(t["comp"])
    print(f"{name:<24s} {'comps':<7s} {U:>10.3e} {mc:9.3f} {U / mc / 1e6:9.3f} {mp:9.3f} {mp / mc:6.2f} {(max(t['call']) - min(t['call'])) / mc:7.2f}")
    torch.cuda.empty_cache()


def main():
    from kmers_amd.api import Context

    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    ctx = Context(0)
    L = 150
    print(f"count_unitig_components (labels, ids and records, no mask) beside its torch composition; {n:.0e} reads of {L} bp, the batch's own table, "
          f"unitigs and links; median of {reps} alternating wall-clock runs each (ms); Gitems/s = unitigs / call ms / 1e6; ratio = comp / call; "
          f"spread = (max - min) / median of the call's runs; MI355X")
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
    ctx.close()


if __name__ == "__main__":
    main()
