"""dev tool: set algebra and comparison of two count tables against what a caller could already write, alternating the two in one
process so both see the same device state; each pair is checked equal before anything is timed.
  kmx_count_setop INTERSECT / SUBTRACT / COUNTER_SUBTRACT   vs torch.searchsorted + gather + compare + boolean indexing
  kmx_count_setop UNION / SYMDIFF                            vs torch.cat + stable sort + run heads
  kmx_count_setop UNION / SUM                                vs kmx_count_merge of the same build
  kmx_count_setop INTERSECT / RIGHT                          vs kmx_count_lookup membership + boolean indexing
  kmx_count_compare                                          vs the sums of the torch compositions above
The two-word calls (k = 47) have no composition in torch: their time per input entry is reported beside the one-word call's.
Times are wall-clock medians of synchronised calls (ms); ns/entry is per INPUT entry (n_a + n_b).  GB/s is the byte MODEL of
DESIGN 4.6.3 over the call's time (one-word keys: count pass 8 n, write pass 16 n in and 16 n_out out; two-word: 16 n, 24 n, 24 n_out),
not a counter reading.  Output: profiles/r10_count_setop_bench.txt.
  python tools/bench_count_setop.py [n_reads, default 1e7] [reps, default 5]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from kmers_amd import _lib
from kmers_amd.api import Context

OPS = {"intersect": _lib.SETOP_INTERSECT, "union": _lib.SETOP_UNION, "subtract": _lib.SETOP_SUBTRACT, "symdiff": _lib.SETOP_SYMDIFF,
       "counter_subtract": _lib.SETOP_COUNTER_SUBTRACT}


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def race(name, new, comp, reps, n_in, model_bytes=None):
    """check equal, then alternate; prints one row; comp None = nothing to race.  Returns (median of new, speed-up or None)."""
    _, a = timed(new)
    if comp is not None:
        _, b = timed(comp)
        same = all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))
        del b
        if not same:
            print(f"{name:<62s} MISMATCH: the call and its composition differ; not timed")
            return None, None
    if model_bytes is not None and callable(model_bytes):
        model_bytes = model_bytes(a)
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
    gbs = f"{model_bytes / mn / 1e6:8.0f}" if model_bytes else f"{'-':>8s}"
    if comp is not None:
        mc = statistics.median(tc)
        print(f"{name:<62s} {n_in:>10.3e} {mn:9.2f} {mc:9.2f} {mc / mn:6.2f} {mn * 1e6 / max(n_in, 1):9.3f} {gbs} {spread:7.2f}")
    else:
        mc = None
        print(f"{name:<62s} {n_in:>10.3e} {mn:9.2f} {'-':>9s} {'-':>6s} {mn * 1e6 / max(n_in, 1):9.3f} {gbs} {spread:7.2f}")
    torch.cuda.empty_cache()
    return mn, (mc / mn if mc is not None else None)


# ---------------------------------------------------------------- the compositions (one-word keys below 2^62: signed order = unsigned)
def _member(ka, kb):
    """for every key of a: is it in b, and where"""
    idx = torch.searchsorted(kb, ka).clamp_(max=max(kb.numel() - 1, 0))
    return kb[idx] == ka, idx


def torch_intersect(ka, ca, kb, cb, rule):
    hit, idx = _member(ka, kb)
    x, y = ca[hit], cb[idx[hit]]
    c = {_lib.RULE_SUM: lambda: x + y, _lib.RULE_MIN: lambda: torch.minimum(x, y), _lib.RULE_MAX: lambda: torch.maximum(x, y),
         _lib.RULE_LEFT: lambda: x, _lib.RULE_RIGHT: lambda: y}[rule]()
    return ka[hit], c


def torch_subtract(ka, ca, kb, cb):
    hit, _ = _member(ka, kb)
    return ka[~hit], ca[~hit]


def torch_counter_subtract(ka, ca, kb, cb):
    hit, idx = _member(ka, kb)
    y = torch.where(hit, cb[idx], torch.zeros_like(ca))
    keep = ca > y
    return ka[keep], (ca - y)[keep]


def _merged(ka, ca, kb, cb):
    k, order = torch.sort(torch.cat([ka, kb]), stable=True)
    c = torch.cat([ca, cb])[order]
    head = torch.ones_like(k, dtype=torch.bool)
    head[1:] = k[1:] != k[:-1]
    twin = torch.zeros_like(head)          # a head whose successor is its equal: the key both tables hold
    twin[:-1] = ~head[1:]
    return k, c, head, twin


def torch_union(ka, ca, kb, cb, rule):
    k, c, head, twin = _merged(ka, ca, kb, cb)
    nxt = torch.roll(c, -1)
    both = {_lib.RULE_SUM: lambda: c + nxt, _lib.RULE_MIN: lambda: torch.minimum(c, nxt), _lib.RULE_MAX: lambda: torch.maximum(c, nxt),
            _lib.RULE_LEFT: lambda: c, _lib.RULE_RIGHT: lambda: nxt}[rule]()
    return k[head], torch.where(twin, both, c)[head]


def torch_symdiff(ka, ca, kb, cb):
    k, c, head, twin = _merged(ka, ca, kb, cb)
    single = head & ~twin
    return k[single], c[single]


def lookup_intersect_right(ctx, k):
    def f(ka, kb, cb):
        member = ctx.count_lookup(ka, None, k, kb) != 0
        return kb[member], cb[member]
    return f


def bytes1(n, words):
    """the byte model: keys read by the count pass, keys and counts by the write pass, the result written"""
    return lambda out: 8 * words * n + (8 * words + 8) * n + (8 * words + 8) * int(out[1].numel())


def tables(ctx, n_reads, L, k, shared=True, seed=1):
    """two tables of n_reads reads each; shared: every second read of B is a read of A"""
    a = ctx.gen_reads(n_reads * L, seed=seed)
    b = ctx.gen_reads(n_reads * L, seed=seed + 1)
    if shared:
        b.view(n_reads, L)[::2] = a.view(n_reads, L)[::2]
    cc = ctx.count_canonical if k <= 31 else ctx.count_canonical2
    out = []
    for x in (a, b):
        kk, c = cc(x, n_reads, L, k)
        out += [kk.clone(), c.clone()]
        del kk, c
        torch.cuda.empty_cache()
    return out


def one_word_shape(ctx, label, ka, ca, kb, cb, k, reps, margins):
    n = int(ca.numel() + cb.numel())
    rows = [
        ("intersect / sum   vs searchsorted", lambda: ctx.count_setop(OPS["intersect"], ka, ca, kb, cb, _lib.RULE_SUM),
         lambda: torch_intersect(ka, ca, kb, cb, _lib.RULE_SUM)),
        ("intersect / min   vs searchsorted", lambda: ctx.count_setop(OPS["intersect"], ka, ca, kb, cb, _lib.RULE_MIN),
         lambda: torch_intersect(ka, ca, kb, cb, _lib.RULE_MIN)),
        ("subtract          vs searchsorted", lambda: ctx.count_setop(OPS["subtract"], ka, ca, kb, None, 0), lambda: torch_subtract(ka, ca, kb, cb)),
        ("counter_subtract  vs searchsorted", lambda: ctx.count_setop(OPS["counter_subtract"], ka, ca, kb, cb, 0),
         lambda: torch_counter_subtract(ka, ca, kb, cb)),
        ("union / sum       vs cat + sort", lambda: ctx.count_setop(OPS["union"], ka, ca, kb, cb, _lib.RULE_SUM),
         lambda: torch_union(ka, ca, kb, cb, _lib.RULE_SUM)),
        ("union / max       vs cat + sort", lambda: ctx.count_setop(OPS["union"], ka, ca, kb, cb, _lib.RULE_MAX),
         lambda: torch_union(ka, ca, kb, cb, _lib.RULE_MAX)),
        ("symdiff           vs cat + sort", lambda: ctx.count_setop(OPS["symdiff"], ka, ca, kb, cb, 0), lambda: torch_symdiff(ka, ca, kb, cb)),
    ]
    for name, new, comp in rows:
        _, sp = race(f"{label} {name}", new, comp, reps, n, bytes1(n, 1))
        if sp is not None:
            margins.append((sp, f"{label} {name}"))
    race(f"{label} union / sum       vs kmx_count_merge", lambda: ctx.count_setop(OPS["union"], ka, ca, kb, cb, _lib.RULE_SUM),
         lambda: ctx.count_merge(ka, ca, kb, cb), reps, n, bytes1(n, 1))
    f = lookup_intersect_right(ctx, k)
    race(f"{label} intersect / right vs lookup + indexing", lambda: ctx.count_setop(OPS["intersect"], ka, None, kb, cb, _lib.RULE_RIGHT),
         lambda: f(ka, kb, cb), reps, n, bytes1(n, 1))

    def cmp_new():
        r = ctx.count_compare(ka, ca, kb, cb)
        return (torch.tensor([r.n_both, r.sum_a_both % 2**63, r.sum_min % 2**63]),)

    def cmp_torch():
        hit, idx = _member(ka, kb)
        x, y = ca[hit], cb[idx[hit]]
        return (torch.tensor([int(hit.sum().item()), int(x.sum().item()) % 2**63, int(torch.minimum(x, y).sum().item()) % 2**63]),)
    _, sp = race(f"{label} compare           vs searchsorted + sums", cmp_new, cmp_torch, reps, n, 16 * n)
    if sp is not None:
        margins.append((sp, f"{label} compare"))


def main():
    n_reads = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    L = 150
    ctx = Context(0)
    print(f"# {torch.cuda.get_device_name(0)}; {n_reads:.1e} reads of {L} bp per table; medians of {reps} synchronised calls, alternating")
    print(f"{'case':<62s} {'entries in':>10s} {'ms':>9s} {'other ms':>9s} {'x':>6s} {'ns/entry':>9s} {'model GB/s':>8s} {'spread':>7s}")
    margins = []
    for k in (31, 21):
        ka, ca, kb, cb = tables(ctx, n_reads, L, k)
        one_word_shape(ctx, f"k={k} half shared", ka, ca, kb, cb, k, reps, margins)
        if k == 31:
            sk, sc = tables(ctx, max(n_reads // 100, 1000), L, k, seed=1)[:2]      # reads of A again: a small table inside a large one
            one_word_shape(ctx, "k=31 small a in large b", sk, sc, kb, cb, k, reps, margins)
            one_word_shape(ctx, "k=31 large a, small b", kb, cb, sk, sc, k, reps, margins)
            del sk, sc
            one_word_shape(ctx, "k=31 identical", ka, ca, ka.clone(), ca.clone(), k, reps, margins)
            del kb, cb
            torch.cuda.empty_cache()
            kb, cb = tables(ctx, n_reads, L, k, shared=False, seed=7)[2:]
            one_word_shape(ctx, "k=31 disjoint", ka, ca, kb, cb, k, reps, margins)
        del ka, ca, kb, cb
        torch.cuda.empty_cache()
    # two-word keys: no composition; per input entry, beside the one-word figures above
    n2 = n_reads // 2
    ka, ca, kb, cb = tables(ctx, n2, L, 47)
    n = int(ca.numel() + cb.numel())
    for name, op, rule in (("intersect / sum", "intersect", _lib.RULE_SUM), ("subtract", "subtract", 0), ("counter_subtract", "counter_subtract", 0),
                           ("union / sum", "union", _lib.RULE_SUM), ("symdiff", "symdiff", 0)):
        race(f"k=47 half shared {name}", lambda: ctx.count_setop2(OPS[op], ka, ca, kb, cb, rule), None, reps, n, bytes1(n, 2))
    race("k=47 half shared union / sum       vs kmx_count_merge2", lambda: ctx.count_setop2(OPS["union"], ka, ca, kb, cb, _lib.RULE_SUM),
         lambda: ctx.count_merge2(ka, ca, kb, cb), reps, n, bytes1(n, 2))
    race("k=47 half shared compare", lambda: (torch.tensor([ctx.count_compare2(ka, ca, kb, cb).n_both]),), None, reps, n, 24 * n)
    if margins:
        sp, name = min(margins)
        print(f"# narrowest margin over a torch composition: {sp:.2f}x ({name}); {sum(1 for s, _ in margins if s <= 1.0)} of {len(margins)} shapes at or below 1.0x")
    ctx.close()


if __name__ == "__main__":
    main()
