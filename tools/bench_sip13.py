"""dev tool: rates of the *_sip13 calls (SipHash-1-3 under std's DefaultHasher / RandomState) next to the Lex rate of the same call,
and a CPU figure for the same hashing: numpy SipHash-1-3 on 16 threads, the hash alone.  That figure is a vectorised numpy
restatement, NOT a native SipHash (which runs at roughly a hundred times its rate): it is a floor for the CPU, not a comparison.
Wall times are CUDA-event medians; the kernel times come from a rocprofv3 --kernel-trace --stats run of this tool.
Output: profiles/r07_sip13_bench.txt.
  python tools/bench_sip13.py [n_reads for reduce / histogram, default 1e8] [n_reads for minimizers, default 1e7]"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from _timing import warm
from kmers_amd import _lib
from kmers_amd.api import Context
from tests import sip13_np

KEY = (0xA5C311F09B2E7D41, 0x3C6EF372FE94F82B)


def timed(f, reps=3):
    warm(f, at_least=3)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def cpu_rate(n_words=1 << 24, threads=16):
    """SipHash-1-3 words per second on `threads` CPU threads (numpy releases the GIL inside its ufuncs)"""
    words = np.random.default_rng(0).integers(0, 2**64, n_words, dtype=np.uint64)
    parts = np.array_split(words, threads * 4)
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda p: sip13_np.siphash13(p, *KEY), parts[:threads]))
        t0 = time.perf_counter()
        list(ex.map(lambda p: sip13_np.siphash13(p, *KEY), parts))
        return n_words / (time.perf_counter() - t0)


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
    nm = int(float(sys.argv[2])) if len(sys.argv) > 2 else 10_000_000
    ctx = Context(0)
    L, k = 150, 31
    W = L - k + 1
    cpu = cpu_rate()
    print(f"CPU figure (numpy SipHash-1-3 of ready words on 16 threads, hash only; not a native implementation): {cpu / 1e9:.3f} G hashes/s")
    bases = ctx.gen_reads(n * L, seed=7)
    rows = []

    def row(name, ms, tot, lex_ms=None):
        r = f"{name:<44s} {ms:9.3f} ms  {tot / ms / 1e9:7.3f} e12 k-mers/s"
        if lex_ms is not None:
            r += f"   | Lex: {lex_ms:8.3f} ms  {tot / lex_ms / 1e9:7.3f} e12/s"
        r += f"   | numpy CPU figure: {tot / cpu * 1e3:9.1f} ms"
        rows.append(r)
        print(r, flush=True)

    tot = n * W
    ms = timed(lambda: ctx.canonical_reduce_sip13(bases, n, L, k, *KEY))
    lex = timed(lambda: ctx.canonical_reduce(bases, n, L, k, _lib.HASH_LEX, k))
    row(f"reduce {n:.0e} x {L} bp k={k} clean", ms, tot, lex)
    dirty = bases.clone()
    rng = np.random.default_rng(7)
    rd = rng.choice(n, n // 50, replace=False)
    dirty[torch.from_numpy((rd * L + rng.integers(0, L, len(rd))).astype(np.int64)).cuda()] = ord("N")
    ms = timed(lambda: ctx.canonical_reduce_sip13(dirty, n, L, k, *KEY))
    lex = timed(lambda: ctx.canonical_reduce(dirty, n, L, k, _lib.HASH_LEX, k))
    row(f"reduce {n:.0e} x {L} bp k={k} 2 % dirty", ms, tot, lex)
    del dirty
    for b in (10, 20):
        c = torch.zeros(1 << b, dtype=torch.int64, device="cuda")
        ms = timed(lambda: ctx.histogram_sip13(bases, n, L, k, b, *KEY, counts=c))
        lex = timed(lambda: ctx.histogram(bases, n, L, k, _lib.HASH_LEX, k, b, counts=c))
        row(f"histogram 2^{b} {n:.0e} x {L} bp k={k}", ms, tot, lex)
    mb = bases[: nm * L]
    tot = nm * W
    ms = timed(lambda: ctx.minimizers_sip13(mb, nm, L, 31, 15, *KEY, check=False))
    lex = timed(lambda: ctx.minimizers(mb, nm, L, 31, 15, _lib.HASH_LEX, 15, check=False))
    row(f"minimizers {nm:.0e} x {L} bp k=31 w=15", ms, tot, lex)
    sv = ctx.seqvec_from_bytes(mb)
    ms = timed(lambda: ctx.seqvec_minimizers_sip13(sv, nm, L, 31, 15, *KEY))
    lex = timed(lambda: ctx.seqvec_minimizers(sv, nm, L, 31, 15, _lib.HASH_LEX, 15))
    row(f"seqvec_minimizers {nm:.0e} x {L} bp k=31 w=15", ms, tot, lex)
    ctx.close()


if __name__ == "__main__":
    main()
