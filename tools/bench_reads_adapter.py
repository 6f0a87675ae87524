"""dev tool: kmx_reads_adapter and kmx_reads_pair_overlap beside torch compositions that produce the same KEEP words, and beside a
plain copy of the bytes a call reads.  One process, so that everything sees the same device state; a call and its composition are
checked equal before anything is timed.
  (a)  kmx_reads_adapter into rows that are there: one adapter (TruSeq, 13 bases), then eight (13 to 33 bases); min_overlap = 3,
       at most 1 mismatch in 10 bases.  A quarter of the reads carry a planted TruSeq adapter at a random position.
  (b)  torch on the device: per adapter base j one pass over the flat batch that adds "base p + j differs" to a mismatch count per
       position, where j is inside the overlap; then the integer test, and the smallest hit per read by a segment minimum.
  (c)  Tensor.copy_ of as many bytes as the call reads (half of them read, half written: the same traffic).
  (d)  kmx_reads_pair_overlap on mates cut from fragments (a quarter shorter than the read: read-through), min_overlap = 30,
       max_mism = 5, 1 in 5; for the uniform batch beside a torch loop over the 2 L - 1 shifts.
Two batches: uniform reads of 150 bp and a ragged mix of 100 .. 160 bp.  All bases are upper-case ACGT, which is what lets the
composition compare bytes.  Times are wall-clock medians of synchronised calls (ms) after three warm-up calls of each, the
contestants alternating.
Output: profiles/reads_adapter_bench.txt.
  python tools/bench_reads_adapter.py [n_reads, default 1e7] [reps, default 5]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

MIN_OVERLAP, ERR = 3, (1, 10)
P_MIN_OVERLAP, P_MAX_MISM, P_ERR = 30, 5, (1, 5)
ONE = ["AGATCGGAAGAGC"]
EIGHT = ["AGATCGGAAGAGC", "CTGTCTCTTATACACATCT", "TGGAATTCTCGGGTGCCAAGG", "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT",
         "GATCGTCGGACTGTAGAACTCTGAAC", "AATGATACGGCGACCACCGAGATCTACAC", "CAAGCAGAAGACGGCATACGAGAT"]


def adapter_keep(bases, offsets, adapters, min_overlap, err):
    """-> KEEP words int64[n]: the smallest hit of any adapter per read, << 32 (no hit: the length); offsets int64[n + 1]"""
    dev = bases.device
    n = offsets.numel() - 1
    total = bases.numel()
    lens = offsets[1:] - offsets[:-1]
    read = torch.repeat_interleave(torch.arange(n, device=dev), lens, output_size=total)
    pos = torch.arange(total, device=dev, dtype=torch.int64) + offsets[0]
    rem = (offsets[1:][read] - pos).clamp_(max=255).to(torch.int16)     # bases from here to the read's end
    p_in = (pos - offsets[:-1][read]).to(torch.int32)                     # the position in its read
    del pos
    best = lens.clone()
    flat = bases[int(offsets[0]):int(offsets[0]) + total]
    for ad in adapters:
        a = torch.tensor(list(ad.encode()), dtype=torch.uint8, device=dev)
        A = a.numel()
        padded = torch.cat([flat, torch.zeros(A, dtype=torch.uint8, device=dev)])
        m = torch.zeros(total, dtype=torch.int16, device=dev)
        for j in range(A):
            m += ((padded[j:j + total] != a[j]) & (rem > j)).to(torch.int16)
        nn = rem.clamp(max=A)
        hit = (nn >= min_overlap) & (m.to(torch.int32) * err[1] <= nn.to(torch.int32) * err[0])
        first = torch.where(hit, p_in, torch.full_like(p_in, 2**31 - 1)).to(torch.int64)
        best = torch.minimum(best, torch.full((n,), 2**31 - 1, device=dev, dtype=torch.int64).scatter_reduce_(0, read, first, "amin", include_self=True))
        del m, hit, first, padded
    return best << 32


def pair_keep(m1, m2, L, min_overlap, max_mism, err):
    """uniform mates [n, L] -> (KEEP1, KEEP2) words int64[n]: a loop over the shifts, the longest overlap, then the largest d"""
    comp = torch.zeros(256, dtype=torch.uint8, device=m1.device)
    comp[list(b"ACGT")] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=m1.device)
    x, y = m1.view(-1, L), comp[m2.view(-1, L).flip(1).long()]
    best = torch.zeros(x.shape[0], dtype=torch.int64, device=m1.device)   # n << 32 | insert
    for d in range(-(L - 1), L):
        nn = L - abs(d)
        if nn < min_overlap:
            continue
        xs, ys = max(d, 0), max(-d, 0)
        m = (x[:, xs:xs + nn] != y[:, ys:ys + nn]).sum(1)
        hit = (m <= max_mism) & (m * err[1] <= nn * err[0])
        best = torch.maximum(best, torch.where(hit, (nn << 32) | (d + L), 0))
    ins = best & 0xFFFFFFFF
    keep = torch.where(best > 0, ins.clamp(max=L), torch.full_like(ins, L)) << 32
    return keep, keep


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median_ms(fs, reps):
    for f in fs:
        for _ in range(3):
            _, o = timed(f)
            del o
    t = [[] for _ in fs]
    for _ in range(reps):
        for i, f in enumerate(fs):
            ms, o = timed(f)
            t[i].append(ms)
            del o
    return [statistics.median(x) for x in t], [(max(x) - min(x)) / statistics.median(x) for x in t]


def copy_pair(nbytes, dev):
    """copy_ of nbytes / 2 moves nbytes"""
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    return lambda: dst.copy_(src)


def adapter_race(ctx, name, bases, n, read_len, offsets, adapters, reps):
    from kmers_amd import _lib
    from kmers_amd.api import _ptr

    dev = ctx.device
    flat = offsets if offsets is not None else torch.arange(n + 1, device=dev, dtype=torch.int64) * read_len
    rows = torch.empty(n * _lib.RA_WORDS, dtype=torch.int64, device=dev)
    call = lambda: ctx.reads_adapter(bases, n, read_len, adapters, MIN_OVERLAP, ERR, offsets, out=rows)   # noqa: E731
    comp = lambda: adapter_keep(bases, flat, adapters, MIN_OVERLAP, ERR)                                  # noqa: E731
    _, got = timed(call)
    _, want = timed(comp)
    same = torch.equal(got[:, _lib.RA_KEEP], want)
    n_hit = int((got[:, _lib.RA_HIT] != 0).sum())
    del want, got
    torch.cuda.empty_cache()
    if not same:
        print(f"{name:<8s} {len(adapters)} adapters MISMATCH: the call and its composition differ; not timed")
        return
    nb = bases.numel()
    with torch.cuda.stream(ctx.stream):
        (a, b, c), spread = median_ms([call, comp, copy_pair(nb + 32 * n, dev)], reps)
    print(f"{name:<8s} {len(adapters):>3d} {n:>10.3e} {nb:>10.3e} {n_hit / n:7.3f} {a:8.3f} {(nb + 32 * n) / a / 1e6:8.1f} {b:10.3f} {c:8.3f} "
          f"{(nb + 32 * n) / c / 1e6:8.1f} {b / a:8.2f} {c / a:7.2f} {spread[0]:7.2f}")
    torch.cuda.empty_cache()


def pair_race(ctx, name, m1, m2, n, L1, L2, o1, o2, reps):
    from kmers_amd import _lib

    dev = ctx.device
    rows = torch.empty(n * _lib.RP_WORDS, dtype=torch.int64, device=dev)
    call = lambda: ctx.reads_pair_overlap(m1, m2, n, L1, L2, o1, o2, P_MIN_OVERLAP, P_MAX_MISM, P_ERR, out=rows)   # noqa: E731
    _, got = timed(call)
    n_hit = int((got[:, _lib.RP_INSERT] != 0).sum())
    fs = [call, copy_pair(m1.numel() + m2.numel() + 32 * n, dev)]
    if o1 is None:
        comp = lambda: pair_keep(m1, m2, L1, P_MIN_OVERLAP, P_MAX_MISM, P_ERR)   # noqa: E731
        _, want = timed(comp)
        if not (torch.equal(got[:, _lib.RP_KEEP1], want[0]) and torch.equal(got[:, _lib.RP_KEEP2], want[1])):
            print(f"{name:<8s} pairs MISMATCH: the call and its composition differ; not timed")
            return
        del want
        fs.append(comp)
    del got
    torch.cuda.empty_cache()
    with torch.cuda.stream(ctx.stream):
        t, spread = median_ms(fs, reps)
    moved = m1.numel() + m2.numel() + 32 * n
    comp_txt = f"{t[2]:10.3f} {t[2] / t[0]:8.2f}" if len(t) > 2 else f"{'-':>10s} {'-':>8s}"
    print(f"{name:<8s} pairs {n:>10.3e} {moved:>10.3e} {n_hit / n:7.3f} {t[0]:8.3f} {moved / t[0] / 1e6:8.1f} {comp_txt} {t[1]:8.3f} {t[1] / t[0]:7.2f} "
          f"{spread[0]:7.2f}")
    torch.cuda.empty_cache()


def plant(bases, flat, n, adapter, g):
    """the adapter over a quarter of the reads, from a random position on (cut at the read's end)"""
    dev = bases.device
    a = torch.tensor(list(adapter.encode()), dtype=torch.uint8, device=dev)
    which = torch.nonzero(torch.rand(n, device=dev, generator=g) < 0.25).squeeze(1)
    lens = (flat[1:] - flat[:-1])[which]
    p = (torch.rand(which.numel(), device=dev, generator=g) * lens).long()
    for j in range(a.numel()):
        ok = p + j < lens
        bases[(flat[:-1][which] + p + j)[ok]] = a[j]


def make_mates(ctx, n, flat1, flat2, g):
    """mates of fragments: a quarter of the inserts shorter than the reads (read-through into random bases), the others up to the sum
    of the two lengths (from a full overlap down to none)"""
    dev = ctx.device
    l1, l2 = flat1[1:] - flat1[:-1], flat2[1:] - flat2[:-1]
    short = torch.rand(n, device=dev, generator=g) < 0.25
    u = torch.rand(n, device=dev, generator=g)
    ins = torch.where(short, 40 + (u * (torch.minimum(l1, l2) - 40)).long(), torch.maximum(l1, l2) + (u * torch.minimum(l1, l2)).long())
    width = int((l1 + l2).max())
    m1 = ctx.gen_reads(int(flat1[-1]), seed=0xF00D)
    m2 = ctx.gen_reads(int(flat2[-1]), seed=0xFEED)
    comp = torch.zeros(256, dtype=torch.uint8, device=dev)
    comp[list(b"ACGT")] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=dev)
    chunk = 1 << 20
    for lo in range(0, n, chunk):   # the fragments, a chunk of pairs at a time
        hi = min(lo + chunk, n)
        frag = ctx.gen_reads((hi - lo) * width, seed=0xABCD + lo).view(hi - lo, width)
        for mate, flat, ln, rc in ((m1, flat1, l1, False), (m2, flat2, l2, True)):
            L = int(ln[lo:hi].max())
            j = torch.arange(L, device=dev)[None, :]
            inside = (j < ln[lo:hi, None]) & (j < ins[lo:hi, None])
            src = (ins[lo:hi, None] - 1 - j) if rc else j.expand(hi - lo, L)
            val = torch.gather(frag, 1, src.clamp(0, width - 1))
            val = comp[val.long()] if rc else val
            dst = flat[lo:hi, None] + j
            mate[dst[inside]] = val[inside]
    return m1, m2


def main():
    from kmers_amd.api import Context

    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = Context(0)
    dev = ctx.device
    print(f"reads_adapter and reads_pair_overlap beside torch compositions of their KEEP words and a plain copy; {n:.0e} reads; adapters: min_overlap = "
          f"{MIN_OVERLAP}, {ERR[0]} mismatch in {ERR[1]}; pairs: min_overlap = {P_MIN_OVERLAP}, max_mism = {P_MAX_MISM}, {P_ERR[0]} in {P_ERR[1]}; median of "
          f"{reps} alternating wall-clock runs each (ms) after 3 warm-up calls; call = the Context method into given rows, GB/s = (the bases + 32 bytes "
          f"per read) / time; comp = the torch composition; copy = Tensor.copy_ moving as many bytes, GB/s = bytes moved / time; b/a = comp / call, "
          f"c/a = copy / call; hit = share of the reads (pairs) with a hit; spread = (max - min) / median of the call's runs; MI355X")
    print(f"{'batch':<8s} {'ad':>3s} {'reads':>10s} {'bytes':>10s} {'hit':>7s} {'call':>8s} {'GB/s':>8s} {'comp':>10s} {'copy':>8s} {'GB/s':>8s} {'b/a':>8s} "
          f"{'c/a':>7s} {'spread':>7s}")
    g = torch.Generator(device=dev).manual_seed(11)
    batches = []
    for name, lo, hi in (("150 bp", 150, 150), ("100-160", 100, 160)):
        if lo == hi:
            offsets, read_len = None, lo
            flat = torch.arange(n + 1, device=dev, dtype=torch.int64) * lo
        else:
            lens = torch.randint(lo, hi + 1, (n,), device=dev, generator=g)
            offsets = torch.zeros(n + 1, device=dev, dtype=torch.int64)
            torch.cumsum(lens, 0, out=offsets[1:])
            flat, read_len = offsets, hi
        bases = ctx.gen_reads(int(flat[-1]), seed=0xBEEF)
        plant(bases, flat, n, ONE[0], g)
        for adapters in (ONE, EIGHT):
            adapter_race(ctx, name, bases, n, read_len, offsets, adapters, reps)
        del bases
        torch.cuda.empty_cache()
        batches.append((name, read_len, offsets, flat))
    print(f"{'batch':<8s} {'':>5s} {'pairs':>10s} {'bytes':>10s} {'hit':>7s} {'call':>8s} {'GB/s':>8s} {'comp':>10s} {'b/a':>8s} {'copy':>8s} {'c/a':>7s} {'spread':>7s}")
    for name, read_len, offsets, flat in batches:
        if offsets is None:
            flat2, o2 = flat, None
        else:
            lens2 = torch.randint(100, 161, (n,), device=dev, generator=g)
            o2 = torch.zeros(n + 1, device=dev, dtype=torch.int64)
            torch.cumsum(lens2, 0, out=o2[1:])
            flat2 = o2
        m1, m2 = make_mates(ctx, n, flat, flat2, g)
        pair_race(ctx, name, m1, m2, n, read_len, read_len, offsets, o2, reps)
        del m1, m2
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
