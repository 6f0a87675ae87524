"""dev tool: kmx_reads_complexity beside a torch composition that produces the same KEEP, AC, GT and DIFF words and the same masked
bytes, beside a plain copy of the bytes the call moves, and beside kmx_reads_quality on the same batch.  One process, so that
everything sees the same device state; the call and its composition are checked equal before anything is timed.
  (a)  kmx_reads_complexity: G tails only (fastp --trim_poly_g) and all four letters at both ends
       (--trim_poly_x), each with and without the masked copy; min_len = 10, at most 1 other base in 10, penalty 2, dust_max = 122.
       A tenth of the reads carry a planted G tail of 10 to 59 bases, a twentieth a dinucleotide repeat of 40 to 99 bases.
  (b)  torch on the device: per letter and end one running sum of "is not X" over the flat batch, the rule on every position and a
       segment maximum of a packed key; the triplets of every window through one index_add_ into a (windows x 64) table.  It holds
       a few hundred bytes per base, so it runs -- and is raced against the call -- on the first `sub` reads of the batch.
  (c)  Tensor.copy_ of as many bytes as the call moves (the bases read, the masked bytes and 64 bytes of row per read written).
  (d)  kmx_reads_quality (min_q 20, trim_q 20, k 31, its masked copy and rows) on the same bases with random quality bytes.
Two batches: uniform reads of 150 bp and a ragged mix of 100 .. 160 bp.  All bases are upper-case ACGT, which is what lets the
composition compare bytes.  Times are wall-clock medians of synchronised calls (ms) after three warm-up calls of each, the
contestants alternating.
Output: profiles/reads_complexity_bench.txt.
  python tools/bench_reads_complexity.py [n_reads, default 1e7] [reps, default 5] [sub, default 5e5]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

MIN_LEN, ERR, PENALTY, DUST_MAX = 10, (1, 10), 2, 122
CONFIGS = [("G tail", "G", ""), ("all x 2", "ACGT", "ACGT")]


def composition(bases, flat, tail, head, min_len, err, penalty, dust_max, want_mask):
    """-> (KEEP, AC, GT, DIFF words int64[n], masked uint8 or None) of the reads at flat int64[n + 1] (upper-case ACGT, reads below
    2^16 bases)"""
    dev = bases.device
    n = flat.numel() - 1
    base, total = int(flat[0]), int(flat[-1] - flat[0])
    b = bases[base:base + total]
    lens = flat[1:] - flat[:-1]
    assert int(lens.max()) < 2**16
    read = torch.repeat_interleave(torch.arange(n, device=dev), lens, output_size=total)
    pos = torch.arange(total, device=dev, dtype=torch.int64)
    start, end = (flat[:-1] - base)[read], (flat[1:] - base)[read]
    p = pos - start
    code = torch.full((256,), 4, dtype=torch.int64, device=dev)
    code[list(b"ACGT")] = torch.arange(4, device=dev)
    c = code[b.long()]
    valid = c < 4
    cnt = [torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, read, (c == x).long()) for x in range(4)]
    pair = valid[:-1] & valid[1:] & (read[:-1] == read[1:])
    P = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, read[:-1], pair.long())
    D = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, read[:-1], (pair & (c[:-1] != c[1:])).long())
    ends = []
    for letters, is_tail in ((tail, True), (head, False)):
        best = torch.zeros(n, dtype=torch.int64, device=dev)
        for x in range(4):
            if "ACGT"[x] not in letters:
                continue
            miss = (c != x).long()
            run = torch.cumsum(miss, 0)
            if is_tail:
                m, nn = run[end - 1] - run + miss, end - pos
            else:
                m, nn = run - run[start] + miss[start], p + 1
            ok = (c == x) & (nn >= min_len) & (m * err[1] <= err[0] * nn)
            key = torch.where(ok, ((nn - (penalty + 1) * m + 2**25) << 20) | (nn << 4) | (3 - x), torch.zeros_like(nn))
            best.scatter_reduce_(0, read, key, "amax", include_self=True)
            del miss, run, m, nn, ok, key
        ends.append((best >> 4) & 0xFFFF)
    t, h = ends
    keep = torch.where(h + t >= lens, torch.zeros_like(lens), h | ((lens - h - t) << 32))
    masked = None
    if want_mask:
        W = torch.where(lens == 0, 0, torch.where(lens <= 64, 1, (lens - 33) // 32 + 1))
        first = torch.cumsum(W, 0) - W                                     # the first window of every read
        two = (c[:-2] < 4) & (c[1:-1] < 4) & (c[2:] < 4) & (p[:-2] + 2 < lens[read[:-2]])
        spell = (c[:-2] + 4 * c[1:-1] + 16 * c[2:]).clamp(max=63)
        j = p[:-2] // 32
        hist = torch.zeros(int(W.sum()) * 64, dtype=torch.int32, device=dev)
        ones = torch.ones(1, dtype=torch.int32, device=dev)
        for jj, ok in ((j, two & (j < W[read[:-2]])), (j - 1, two & (j >= 1) & (p[:-2] % 32 < 30))):
            hist.index_add_(0, ((first[read[:-2]] + jj) * 64 + spell)[ok], ones.expand(int(ok.sum())))
        dusty = (hist * (hist - 1) // 2).view(-1, 64).sum(1) > dust_max
        dusty = torch.cat([dusty, torch.zeros(1, dtype=torch.bool, device=dev)])
        last = dusty.numel() - 1
        j, w0 = p // 32, first[read]
        here = torch.where(j < W[read], w0 + j, torch.full_like(j, last))
        before = torch.where(j >= 1, w0 + j - 1, torch.full_like(j, last))
        masked = torch.where(dusty[here] | dusty[before], torch.full_like(b, ord("N")), b)
    return keep, cnt[0] | (cnt[1] << 32), cnt[2] | (cnt[3] << 32), D | (P << 32), masked


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


def plant(bases, flat, n, g):
    """a G tail of 10 .. 59 bases on a tenth of the reads, (AC)n of 40 .. 99 bases somewhere in a twentieth"""
    dev = bases.device
    lens = flat[1:] - flat[:-1]
    for share, lo, hi, unit, at_end in ((0.10, 10, 60, b"G", True), (0.05, 40, 100, b"AC", False)):
        which = torch.nonzero(torch.rand(n, device=dev, generator=g) < share).squeeze(1)
        ln = lens[which]
        run = torch.minimum(torch.randint(lo, hi, (which.numel(),), device=dev, generator=g), ln)
        p = ln - run if at_end else (torch.rand(which.numel(), device=dev, generator=g) * (ln - run + 1)).long()
        u = torch.tensor(list(unit), dtype=torch.uint8, device=dev)
        for j in range(hi):
            ok = j < run
            bases[(flat[:-1][which] + p + j)[ok]] = u[j % len(unit)]


def race(ctx, name, bases, quals, n, read_len, offsets, flat, sub, reps):
    from kmers_amd import _lib

    dev = ctx.device
    nb = int(flat[-1] - flat[0])
    sflat = flat[:sub + 1]
    soff = None if offsets is None else offsets[:sub + 1]
    snb = int(sflat[-1])
    out = torch.empty_like(bases)
    with torch.cuda.stream(ctx.stream):
        (q_ms,), _ = median_ms([lambda: ctx.reads_quality(bases, quals, n, read_len, 20, 20, 31, offsets=offsets, out=out)], reps)
    for label, tail, head in CONFIGS:
        for mask in (False, True):
            call = lambda: ctx.reads_complexity(bases, n, read_len, tail, head, MIN_LEN, ERR, PENALTY, DUST_MAX, offsets, mask=mask, out=out)   # noqa: E731
            scall = lambda: ctx.reads_complexity(bases, sub, read_len, tail, head, MIN_LEN, ERR, PENALTY, DUST_MAX, soff, mask=mask, out=out)   # noqa: E731
            comp = lambda: composition(bases, sflat, tail, head, MIN_LEN, ERR, PENALTY, DUST_MAX, mask)                                       # noqa: E731
            _, (gm, got) = timed(scall)
            _, want = timed(comp)
            same = all(torch.equal(got[:, w], want[i]) for i, w in enumerate((_lib.RX_KEEP, _lib.RX_AC, _lib.RX_GT, _lib.RX_DIFF)))
            if mask:
                same = same and torch.equal(gm[:snb], want[4])
            _, (gm, got) = timed(call)
            n_tail = int((got[:, _lib.RX_TAIL] != 0).sum())
            n_dusty = int(((got[:, _lib.RX_DUST] >> 32) != 0).sum())
            del want, got, gm
            torch.cuda.empty_cache()
            if not same:
                print(f"{name:<8s} {label:<8s} mask={int(mask)} MISMATCH: the call and its composition differ; not timed")
                continue
            moved = nb * (2 if mask else 1) + 64 * n
            src, dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            with torch.cuda.stream(ctx.stream):
                (a, c, sa, sb), spread = median_ms([call, lambda: dst.copy_(src), scall, comp], reps)
            print(f"{name:<8s} {label:<8s} {int(mask):>4d} {n:>9.2e} {moved:>9.2e} {n_tail / n:6.3f} {n_dusty / n:6.3f} {a:8.3f} {moved / a / 1e6:7.1f} "
                  f"{c:8.3f} {c / a:6.2f} {q_ms:8.3f} {q_ms / a:6.2f} {sub:>8.1e} {sa:8.3f} {sb:10.3f} {sb / sa:8.1f} {spread[0]:6.2f}")
            del src, dst
            torch.cuda.empty_cache()


def main():
    from kmers_amd.api import Context

    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    sub = min(n, int(float(sys.argv[3])) if len(sys.argv) > 3 else 500_000)
    ctx = Context(0)
    dev = ctx.device
    print(f"reads_complexity beside a torch composition of its KEEP, AC, GT, DIFF words and masked bytes, a plain copy and reads_quality; "
          f"{n:.0e} reads; min_len = {MIN_LEN}, {ERR[0]} other base in {ERR[1]}, penalty {PENALTY}, dust_max = {DUST_MAX}; median of {reps} "
          f"alternating wall-clock runs each (ms) after 3 warm-up calls; call = the Context method, GB/s = (bases read + masked bytes + 64 bytes "
          f"of row per read) / time; copy = Tensor.copy_ moving as many bytes, c/a = copy / call; qual = reads_quality with its masked copy and "
          f"rows on the same batch, q/a = qual / call; sub = the reads the composition holds: s.call and s.comp are the call and the composition "
          f"on those, b/a = s.comp / s.call; tail / dusty = share of the reads with a tail / a DUSTY window; spread = (max - min) / median of "
          f"the call's runs; MI355X")
    print(f"{'batch':<8s} {'letters':<8s} {'mask':>4s} {'reads':>9s} {'bytes':>9s} {'tail':>6s} {'dusty':>6s} {'call':>8s} {'GB/s':>7s} {'copy':>8s} "
          f"{'c/a':>6s} {'qual':>8s} {'q/a':>6s} {'sub':>8s} {'s.call':>8s} {'s.comp':>10s} {'b/a':>8s} {'spread':>6s}")
    g = torch.Generator(device=dev).manual_seed(13)
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
        plant(bases, flat, n, g)
        quals = torch.randint(33 + 2, 33 + 41, (int(flat[-1]),), device=dev, dtype=torch.uint8, generator=g)
        race(ctx, name, bases, quals, n, read_len, offsets, flat, sub, reps)
        del bases, quals
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
