"""dev tool: the count-table queries against what a caller could already write in torch, alternating the two in one process so both
see the same device state; each pair is checked equal before anything is timed.
  kmx_count_lookup        vs torch.searchsorted + gather + compare (on canonical_windows output held on the device)
  kmx_count_lookup_reads  vs canonical_windows -> torch.searchsorted + gather + compare, flags applied
  kmx_count_spectrum      vs torch.bincount of the clamped counts
  kmx_count_filter        vs boolean indexing
The two-word calls (k = 47) have no composition in torch (no 128-bit searchsorted): their time per query is reported beside the
one-word call's on the same reads.  Times are wall-clock medians of synchronised calls (ms).  Output: profiles/r09_count_query_bench.txt.
  python tools/bench_count_query.py [n_reads, default 1e7] [reps, default 5]

Bytes per query are a MODEL, not a counter reading: with the directory a query reads its word and flag (9; the reads form 17 more
for the windows written and read back), two adjacent directory entries (one 64-byte sector), the bin (one or two 64-byte sectors of
keys; two-word keys: 128-byte lines), one count (a 64-byte sector) and writes 8; the directory's build adds 8 * words * n / n_query.
A plain search adds one sector per step below the levels the caches hold."""
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


def race(name, new, comp, reps, unit_n, extra=""):
    """check equal, then alternate; prints one row; comp None = nothing to race"""
    _, a = timed(new)
    if comp is not None:
        _, b = timed(comp)
        same = all(torch.equal(x, y) for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)))
        del b
        if not same:
            print(f"{name:<58s} MISMATCH: the call and its composition differ; not timed")
            return None
    del a
    tn, tc = [], []
    for _ in range(reps):
        t, o = timed(new)
        tn.append(t)
        del o
        if comp is not None:
            t, o = timed(comp)
            tc.append(t)
            del o
    mn = statistics.median(tn)
    spread = (max(tn) - min(tn)) / mn
    if comp is not None:
        mc = statistics.median(tc)
        print(f"{name:<58s} {unit_n:>10.3e} {mn:9.2f} {mc:9.2f} {mc / mn:6.2f} {mn * 1e6 / max(unit_n, 1):9.3f} {spread:7.2f} {extra}")
    else:
        print(f"{name:<58s} {unit_n:>10.3e} {mn:9.2f} {'-':>9s} {'-':>6s} {mn * 1e6 / max(unit_n, 1):9.3f} {spread:7.2f} {extra}")
    torch.cuda.empty_cache()
    return mn


def searchsorted_lookup(km, cnt, canon, flags):
    idx = torch.searchsorted(km, canon).clamp_(max=km.numel() - 1)      # (keys below 2^62: signed order = unsigned order)
    hit = km[idx] == canon
    if flags is not None:
        hit &= (flags & 1) != 0
    return torch.where(hit, cnt[idx], torch.zeros_like(canon))


def uses_directory(n, nq, words):
    """the library's choice restated (count_lookup_wants_dir, count_lookup_dir_bytes in kmx_count_query.hip; keep the two in step):
    enough queries to pay for the pass over the keys, 4-byte entries.  The tool sets no work-buffer limit, so the cap does not bind."""
    return n > 8 and nq >= words * n // 64 and n < 2**32


def model_bytes(n, nq, words, reads_form, with_dir):
    b = 8.0 * words + 1.0 + 8.0 + (8.0 * words + 1.0 + (8.0 if words == 2 else 0.0) if reads_form else 0.0)
    b += 64.0 + (64.0 if words == 1 else 128.0) * 1.5 + 64.0
    if with_dir:
        b += 8.0 * words * n / max(nq, 1)
    return b


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = Context(0)
    rng = np.random.default_rng(11)
    L = 150
    print(f"count-table queries vs their torch compositions; table and queries of {n:.0e} reads each, half the query reads shared with the "
          f"table's; median of {reps} alternating wall-clock runs each (ms); spread = (max - min) / median of the call's runs; MI355X")
    print(f"{'shape':<58s} {'items':>10s} {'call ms':>9s} {'comp ms':>9s} {'ratio':>6s} {'ns/item':>9s} {'spread':>7s} notes")
    g = torch.Generator(device=ctx.device).manual_seed(3)
    a = ctx.gen_reads(n * L, seed=0xC0FFEE)
    b = ctx.gen_reads(n * L, seed=0xBEEF)
    b.view(n, L)[::2] = a.view(n, L)[::2]

    def lookup_rows(tag, k, ta, qb, nq_reads, Lq, off=None, hoff=None, lens=None):
        km, cnt = ctx.count_canonical(ta[0], ta[1], ta[2], k, offsets=ta[3])
        nt = int(km.numel())
        w = ctx.canonical_windows(qb, nq_reads, Lq, k, offsets=off, host_offsets=hoff, want=("canon", "flags"))
        nq = int(w["canon"].numel())
        with_dir = uses_directory(nt, nq, 1)
        note = f"table {nt:.3e}, {'directory' if with_dir else 'plain search'}, model {model_bytes(nt, nq, 1, False, with_dir):.0f} B/query"
        race(f"lookup        {tag}", lambda: ctx.count_lookup(km, cnt, k, w["canon"], w["flags"]),
             lambda: searchsorted_lookup(km, cnt, w["canon"], w["flags"]), reps, nq, note)
        wo = None
        if off is not None:
            wo = ctx.to_device(ctx.win_offsets(nq_reads, Lq, k, hoff))
        del w
        out = ctx.empty(nq, torch.int64)

        def comp():
            ww = ctx.canonical_windows(qb, nq_reads, Lq, k, offsets=off, host_offsets=hoff, want=("canon", "flags"))
            return searchsorted_lookup(km, cnt, ww["canon"], ww["flags"])
        note = f"model {model_bytes(nt, nq, 1, True, with_dir):.0f} B/query"
        t1 = race(f"lookup_reads  {tag}", lambda: ctx.count_lookup_reads(qb, nq_reads, Lq, k, km, cnt, offsets=off, win_offsets=wo, out=out), comp,
                  reps, nq, note)
        del out
        return km, cnt, t1, nq

    km, cnt, t31, nq31 = lookup_rows("150 bp, k = 31", 31, (a, n, L, None), b, n, L)
    # the other side of the cut-over: 1e5 query reads against the same table
    nsm = min(100_000, n)
    lookup_small = b[:nsm * L]
    w = ctx.canonical_windows(lookup_small, nsm, L, 31, want=("canon", "flags"))
    nt, nq = int(km.numel()), int(w["canon"].numel())
    race("lookup        1e5 query reads, k = 31", lambda: ctx.count_lookup(km, cnt, 31, w["canon"], w["flags"]),
         lambda: searchsorted_lookup(km, cnt, w["canon"], w["flags"]), reps, nq,
         f"table {nt:.3e}, {'directory' if uses_directory(nt, nq, 1) else 'plain search'}")
    del w
    race("lookup_reads  1e5 query reads, k = 31", lambda: ctx.count_lookup_reads(lookup_small, nsm, L, 31, km, cnt),
         lambda: searchsorted_lookup(km, cnt, *[ctx.canonical_windows(lookup_small, nsm, L, 31, want=("canon", "flags"))[x] for x in ("canon", "flags")]),
         reps, nq)
    # spectrum and filter on the k = 31 table
    for nb in (256, 65536):
        race(f"spectrum      {nb} bins, k = 31 table", lambda: ctx.count_spectrum(cnt, nb),
             lambda: torch.bincount(cnt.clamp(max=nb - 1), minlength=nb), reps, nt)
    for mn, mx in ((2, 2**64 - 1), (1, 1)):
        race(f"filter        [{mn}, {'max' if mx > 10 else mx}], k = 31 table", lambda: ctx.count_filter(km, cnt, mn, mx),
             lambda: (lambda m: (km[m], cnt[m]))((cnt >= mn) & ((cnt <= mx) if mx < 2**63 else (cnt >= 0))), reps, nt)
    del km, cnt
    torch.cuda.empty_cache()
    lookup_rows("150 bp, k = 21", 21, (a, n, L, None), b, n, L)
    dirty = b.clone()
    rows = torch.nonzero(torch.rand(n, device=ctx.device, generator=g) < 0.02).flatten()
    dirty[rows * L + torch.randint(0, L, (rows.numel(),), device=ctx.device, generator=g)] = ord("N")
    lookup_rows("150 bp, k = 31, 2 % dirty reads", 31, (a, n, L, None), dirty, n, L)
    del dirty
    lens = rng.integers(100, 161, n).astype(np.uint64)
    h_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    rag_a = ctx.gen_reads(int(h_off[-1]), seed=0xFACE)
    rag_b = ctx.gen_reads(int(h_off[-1]), seed=0xD00D)
    half = int(h_off[n // 2])
    rag_b[:half] = rag_a[:half]
    d_off = ctx.to_device(h_off)
    lookup_rows("100-160 bp ragged, k = 31", 31, (rag_a, n, 160, d_off), rag_b, n, 160, d_off, h_off)
    del rag_a, rag_b
    mixed_a, mixed_b = a.clone(), b.clone()
    poly = torch.rand(n, device=ctx.device, generator=g) < 0.9
    mixed_a.view(n, L)[poly] = ord("A")
    mixed_b.view(n, L)[poly] = ord("A")
    km, cnt, _, _ = lookup_rows("150 bp, 90 % of reads all A, k = 31", 31, (mixed_a, n, L, None), mixed_b, n, L)
    nt = int(km.numel())
    race("spectrum      256 bins, 90 % all-A table", lambda: ctx.count_spectrum(cnt, 256), lambda: torch.bincount(cnt.clamp(max=255), minlength=256),
         reps, nt)
    del km, cnt, mixed_a, mixed_b
    torch.cuda.empty_cache()
    # two-word keys: nothing to race; time per query beside the one-word call's on the same reads
    n2 = min(n, 5_000_000)                               # (the two-word counter's working set: 36 bytes per window)
    k2 = 47
    km2, cnt2 = ctx.count_canonical2(a[:n2 * L], n2, L, k2)
    nt2, nq2 = int(cnt2.numel()), n2 * (L - k2 + 1)
    t2 = race(f"lookup_reads2 150 bp, k = 47, {n2:.0e} reads", lambda: ctx.count_lookup_reads2(b[:n2 * L], n2, L, k2, km2, cnt2), None, reps, nq2,
              f"table {nt2:.3e}, model {model_bytes(nt2, nq2, 2, True, uses_directory(nt2, nq2, 2)):.0f} B/query")
    w2 = ctx.canonical_windows2(b[:n2 * L], n2, L, k2)
    del w2["fw"], w2["rc"]
    race("lookup2       150 bp, k = 47 (windows on the device)", lambda: ctx.count_lookup2(km2, cnt2, k2, w2["canon"].view(-1, 2), w2["flags"]), None,
         reps, nq2)
    del w2, km2, cnt2
    km, cnt = ctx.count_canonical(a[:n2 * L], n2, L, 31)
    nq1 = n2 * (L - 31 + 1)
    t1 = race(f"lookup_reads  150 bp, k = 31, {n2:.0e} reads (same reads)", lambda: ctx.count_lookup_reads(b[:n2 * L], n2, L, 31, km, cnt), None, reps,
              nq1, f"table {int(km.numel()):.3e}, model {model_bytes(int(km.numel()), nq1, 1, True, uses_directory(int(km.numel()), nq1, 1)):.0f} B/query")
    if t1 and t2:
        print(f"two-word / one-word time per query on the same reads: {(t2 / nq2) / (t1 / nq1):.2f}")
    held, allocs = ctx.work_buffer_info()
    print(f"work buffer held at the end: {held / 2**30:.2f} GiB ({allocs} allocations)")
    ctx.close()


if __name__ == "__main__":
    main()
