"""dev tool: kmx_reads_pair_merge beside a torch composition that yields the same merged bases and quality bytes, beside the whole
Context.reads_merge_pairs, and beside a plain copy of the bytes the merge reads and writes.  One process, so that everything sees
the same device state; the call and its composition are checked equal before anything is timed.
  (a)  write: kmx_reads_pair_merge into outputs that are there (bases, quality bytes, offsets, rows), the insert words taken by
       stride out of the rows of kmx_reads_pair_overlap: the plan (count, two scans, one round trip to the host, write) and the
       merge kernel.
  (b)  merge: Context.reads_pair_merge, that is the count-only call, the allocation of the outputs and (a).
  (c)  pipe: Context.reads_merge_pairs: overlap, merge and six reads_select.
  (d)  comp: torch on the device, uniform batch only: the pairs in chunks of 2^17 as a [chunk, 2 L - 1] matrix of positions, X and
       the gathered reverse complement, the class rule with torch.where, the merged positions picked out with a boolean mask.
  (e)  copy: Tensor.copy_ moving as many bytes as (a) reads and writes.
Mates are cut from fragments: a quarter of the inserts shorter than the mates (read-through into random bases), the others from the
longer mate's length up to 2.4 shorter mates beyond it, so that about a third of them overlap by 30 bases or more: about half of
all pairs merge.  Mate 2 carries 1 % substitutions; the quality bytes are random in phred 2 .. 41.  All bases are upper-case ACGT,
which is what lets the composition do without the validity classes.  Two batches: uniform mates of 150 bp and a ragged mix of
100 .. 160 bp.  Times are wall-clock medians of synchronised calls (ms) after three warm-up calls of each, the contestants
alternating.
Output: profiles/reads_merge_bench.txt.
  python tools/bench_reads_merge.py [n_pairs, default 1e7] [reps, default 5]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from tools.bench_reads_adapter import copy_pair, median_ms, timed

MIN_OVERLAP, MAX_MISM, ERR = 30, 5, (1, 5)
PHRED, Q_CAP = 33, 41
CHUNK = 1 << 17


def make_mates(ctx, n, flat1, flat2, g):
    """-> (mate 1, mate 2, quality bytes 1, quality bytes 2) of fragments as the text above says"""
    dev = ctx.device
    l1, l2 = flat1[1:] - flat1[:-1], flat2[1:] - flat2[:-1]
    lo, hi = torch.minimum(l1, l2), torch.maximum(l1, l2)
    short = torch.rand(n, device=dev, generator=g) < 0.25
    u = torch.rand(n, device=dev, generator=g)
    ins = torch.where(short, 40 + (u * (lo - 40)).long(), hi + (u * 2.4 * lo).long())
    width = int(ins.max()) + 1
    m1 = ctx.gen_reads(int(flat1[-1]), seed=0xF00D)
    m2 = ctx.gen_reads(int(flat2[-1]), seed=0xFEED)
    comp = torch.zeros(256, dtype=torch.uint8, device=dev)
    comp[list(b"ACGT")] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=dev)
    chunk = 1 << 19
    for a in range(0, n, chunk):   # the fragments, a chunk of pairs at a time
        b = min(a + chunk, n)
        frag = ctx.gen_reads((b - a) * width, seed=0xABCD + a).view(b - a, width)
        for mate, flat, ln, rc in ((m1, flat1, l1, False), (m2, flat2, l2, True)):
            L = int(ln[a:b].max())
            j = torch.arange(L, device=dev)[None, :]
            inside = (j < ln[a:b, None]) & (j < ins[a:b, None])
            src = (ins[a:b, None] - 1 - j) if rc else j.expand(b - a, L)
            val = torch.gather(frag, 1, src.clamp(0, width - 1))
            val = comp[val.long()] if rc else val
            mate[(flat[a:b, None] + j)[inside]] = val[inside]
        del frag
    err = torch.nonzero(torch.rand(m2.numel(), device=dev, generator=g) < 0.01).squeeze(1)   # substitutions in mate 2
    m2[err] = comp[m2[err].long()]
    q1 = torch.randint(PHRED + 2, PHRED + 42, (m1.numel(),), device=dev, generator=g, dtype=torch.uint8)
    q2 = torch.randint(PHRED + 2, PHRED + 42, (m2.numel(),), device=dev, generator=g, dtype=torch.uint8)
    return m1, m2, q1, q2


def merge_comp(m1, m2, q1, q2, insert, L):
    """uniform mates [n, L] of upper-case ACGT -> (merged bases, merged quality bytes), the merged reads back to back"""
    dev = m1.device
    comp = torch.zeros(256, dtype=torch.uint8, device=dev)
    comp[list(b"ACGT")] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=dev)
    W = 2 * L - 1
    pos = torch.arange(W, device=dev)[None, :]
    out_b, out_q = [], []
    for a in range(0, insert.numel(), CHUNK):
        ins = insert[a:a + CHUNK, None]
        n = ins.shape[0]
        ok = (ins > 0) & (ins < 2 * L)
        d = ins - L
        x, xq = m1[a * L:(a + n) * L].view(n, L), q1[a * L:(a + n) * L].view(n, L).to(torch.int16) - PHRED
        y, yq = comp[m2[a * L:(a + n) * L].view(n, L).flip(1).long()], q2[a * L:(a + n) * L].view(n, L).flip(1).to(torch.int16) - PHRED
        pad = torch.zeros(n, W - L, dtype=torch.uint8, device=dev)
        x, xq = torch.cat([x, pad], 1), torch.cat([xq, pad.to(torch.int16)], 1)
        j = (pos - d).clamp(0, L - 1)
        y, yq = torch.gather(y, 1, j), torch.gather(yq, 1, j)
        cx, cy = pos < L, pos >= d.clamp(min=0)
        both = cx & cy
        take = both & (x != y) & (yq > xq)
        base = torch.where(cx & ~take, x, y)
        q = torch.where(both, torch.where(x == y, xq + yq, (xq - yq).abs()).clamp(max=Q_CAP), torch.where(cx, xq, yq))
        keep = ok & (pos < ins)
        out_b.append(base[keep])
        out_q.append((q[keep] + PHRED).to(torch.uint8))
    return torch.cat(out_b), torch.cat(out_q)


def race(ctx, name, m1, m2, q1, q2, n, L1, L2, o1, o2, reps):
    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    dev = ctx.device
    ov = ctx.reads_pair_overlap(m1, m2, n, L1, L2, o1, o2, MIN_OVERLAP, MAX_MISM, ERR)
    insert = ov[:, _lib.RP_INSERT]
    b, q, rows = ctx.reads_pair_merge(m1, m2, n, L1, L2, insert, q1, q2, o1, o2, PHRED, Q_CAP)
    n_bases, n_merged, n_dis = b.n_bases, int((rows[:, _lib.RM_LEN] != 0).sum()), int((rows[:, _lib.RM_OVERLAP] >> 32).sum())
    # (a): the raw call into the outputs of (b)
    r1, r2 = ctx._reads(m1, n, L1, o1), ctx._reads(m2, n, L2, o2)
    nm, nb = C.c_uint64(0), C.c_uint64(0)

    def write():
        ctx._ck(ctx.lib.kmx_reads_pair_merge(ctx._h, C.byref(r1), C.byref(r2), _ptr(q1), _ptr(q2), C.c_void_p(insert.data_ptr()), _lib.RP_WORDS, PHRED, Q_CAP,
                                             _ptr(b.bases), _ptr(q.bases), _ptr(b.offsets), _ptr(rows), n_bases, C.byref(nm), C.byref(nb)))

    merge = lambda: ctx.reads_pair_merge(m1, m2, n, L1, L2, insert, q1, q2, o1, o2, PHRED, Q_CAP)                                    # noqa: E731
    pipe = lambda: ctx.reads_merge_pairs(m1, m2, n, L1, L2, q1, q2, o1, o2, MIN_OVERLAP, MAX_MISM, ERR, PHRED, Q_CAP)                  # noqa: E731
    # the bytes (a) moves: of a pair that merges the part of either mate the merged read uses, and as many quality bytes; the insert word
    # and the offsets of every pair; the merged bases and quality bytes, an offset and a row per pair
    ins = rows[:, _lib.RM_LEN]
    l1 = o1[1:] - o1[:-1] if o1 is not None else torch.full_like(ins, L1)
    l2 = o2[1:] - o2[:-1] if o2 is not None else torch.full_like(ins, L2)
    used = int(((torch.minimum(l1, ins) + torch.minimum(l2, ins)) * (ins != 0)).sum())
    moved = 2 * used + 8 * n + (16 * n if o1 is not None else 0) + (16 * n if o2 is not None else 0) + 2 * n_bases + 8 * n + 32 * n
    del ins, l1, l2
    fs = [write, merge, pipe, copy_pair(moved, dev)]
    if o1 is None:
        comp = lambda: merge_comp(m1, m2, q1, q2, insert, L1)   # noqa: E731
        _, want = timed(comp)
        if not (torch.equal(b.bases, want[0]) and torch.equal(q.bases, want[1])):
            print(f"{name:<8s} MISMATCH: the call and its composition differ; not timed")
            return
        del want
        fs.append(comp)
    torch.cuda.empty_cache()
    with torch.cuda.stream(ctx.stream):
        t, spread = median_ms(fs, reps)
    comp_txt = f"{t[4]:10.3f} {t[4] / t[0]:8.2f}" if len(t) > 4 else f"{'-':>10s} {'-':>8s}"
    print(f"{name:<8s} {n:>10.3e} {moved:>10.3e} {n_merged / n:7.3f} {n_dis / max(n_merged, 1):6.2f} {t[0]:8.3f} {moved / t[0] / 1e6:8.1f} {t[1]:8.3f} "
          f"{t[2]:8.3f} {comp_txt} {t[3]:8.3f} {moved / t[3] / 1e6:8.1f} {t[3] / t[0]:7.2f} {spread[0]:7.2f}")
    torch.cuda.empty_cache()


def main():
    from kmers_amd.api import Context

    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = Context(0)
    dev = ctx.device
    print(f"reads_pair_merge beside a torch composition of the same merged bases and quality bytes, the whole reads_merge_pairs and a plain copy; "
          f"{n:.0e} pairs; overlap: min_overlap = {MIN_OVERLAP}, max_mism = {MAX_MISM}, {ERR[0]} in {ERR[1]}; phred_base = {PHRED}, q_cap = {Q_CAP}; median "
          f"of {reps} alternating wall-clock runs each (ms) after 3 warm-up calls; write = kmx_reads_pair_merge into outputs that are there, GB/s = bytes "
          f"/ time, bytes = what it reads (of the pairs that merge the mates and quality bytes as far as the merged read uses them; insert words, offsets) and writes (bases, quality bytes, offsets, rows); merge = "
          f"Context.reads_pair_merge (count-only call, allocation, write); pipe = Context.reads_merge_pairs; comp = the torch composition, b/a = comp / "
          f"write; copy = Tensor.copy_ moving as many bytes, c/a = copy / write; merged = share of the pairs that merge, dis = disagreeing positions "
          f"per merged pair; spread = (max - min) / median of the write's runs; MI355X")
    print(f"{'batch':<8s} {'pairs':>10s} {'bytes':>10s} {'merged':>7s} {'dis':>6s} {'write':>8s} {'GB/s':>8s} {'merge':>8s} {'pipe':>8s} {'comp':>10s} "
          f"{'b/a':>8s} {'copy':>8s} {'GB/s':>8s} {'c/a':>7s} {'spread':>7s}")
    g = torch.Generator(device=dev).manual_seed(12)
    for name, lo, hi in (("150 bp", 150, 150), ("100-160", 100, 160)):
        layouts = []
        for _ in range(2):
            if lo == hi:
                layouts.append((None, torch.arange(n + 1, device=dev, dtype=torch.int64) * lo))
            else:
                offsets = torch.zeros(n + 1, device=dev, dtype=torch.int64)
                torch.cumsum(torch.randint(lo, hi + 1, (n,), device=dev, generator=g), 0, out=offsets[1:])
                layouts.append((offsets, offsets))
        (o1, flat1), (o2, flat2) = layouts
        m1, m2, q1, q2 = make_mates(ctx, n, flat1, flat2, g)
        race(ctx, name, m1, m2, q1, q2, n, hi, hi, o1, o2, reps)
        del m1, m2, q1, q2
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
