"""Host-side inputs and expectations shared by the count family's GPU tests (tests/test_gpu_count*.py).

* random_reads / dirty / two_batches: the seeded read batches the tests count, look up and compare.
* orc_windows: the oracle's canonical words and flags of a batch, one- or two-word by k.
* table_of: the count table of those windows -- sorted distinct valid words and their counts; two-word keys, rows (low, high),
  ordered as 2k-bit unsigned integers (high word first).
* host_lookup: the count of every query in such a table (lower bound + equality), the yardstick of every exact u64 comparison.
* u64, words, the module-scoped `ctx` fixture (imported by name into each test module).

numpy only: torch and kmers_amd are imported inside the functions that need them.  table_of, host_lookup and the batch makers are
pinned against brute force in tests/test_count_np.py, which needs no GPU.
"""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def ctx():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from kmers_amd.api import Context

    c = Context()
    yield c
    c.close()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def words(k):
    return 1 if k <= 31 else 2


def random_reads(rng, nbytes):
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), nbytes).astype(np.uint8)


def dirty(host, rng, share, n, L):
    h = host.copy()
    for r in np.nonzero(rng.random(n) < share)[0]:
        p = int(rng.integers(0, L))
        h[r * L + p] = ord("N") if r % 3 else ord(">")
    return h


def two_batches(rng, n, L):
    """A and B: every second read of B is a read of A"""
    a = random_reads(rng, n * L)
    b = random_reads(rng, n * L)
    b.reshape(n, L)[::2] = a.reshape(n, L)[::2]
    return a, b


def orc_windows(orc, host, n, L, k, offsets=None):
    """the oracle's canonical words ((windows,) or (windows, 2) uint64) and flags of a batch"""
    f = orc.canonical_windows if k <= 31 else orc.canonical_windows2
    _, _, canon, flags = f(host, n, L, k, offsets=offsets)
    return np.asarray(canon, np.uint64), np.asarray(flags, np.uint8)


def table_of(canon, flags):
    """sorted distinct valid canonical words and their counts, on the host"""
    c = canon[(flags & 1) != 0]
    if c.ndim == 1:
        k_, c_ = np.unique(c, return_counts=True)
        return k_, c_.astype(np.uint64)
    c = c[np.lexsort((c[:, 0], c[:, 1]))]
    head = np.ones(len(c), bool)
    head[1:] = (c[1:] != c[:-1]).any(axis=1)
    idx = np.nonzero(head)[0]
    return c[head], np.diff(np.append(idx, len(c))).astype(np.uint64)


def host_lookup(tk, tc, q, qflags=None):
    """expected answers on the host: lower bound + equality; tc None = membership"""
    n = len(tk)
    out = np.zeros(len(q), np.uint64)
    if n == 0 or len(q) == 0:
        return out
    if tk.ndim == 1:
        i = np.searchsorted(tk, q)
        ic = np.minimum(i, n - 1)
        found = (i < n) & (tk[ic] == q)
    else:
        thi, tlo, qhi, qlo = tk[:, 1], tk[:, 0], q[:, 1], q[:, 0]
        lo = np.searchsorted(thi, qhi, "left")
        hi = np.searchsorted(thi, qhi, "right")
        for _ in range(44):                      # lower bound of the low word inside the run of equal high words
            act = lo < hi
            mid = (lo + hi) // 2
            less = tlo[np.minimum(mid, n - 1)] < qlo
            lo = np.where(act & less, mid + 1, lo)
            hi = np.where(act & ~less, mid, hi)
        ic = np.minimum(lo, n - 1)
        found = (lo < n) & (thi[ic] == qhi) & (tlo[ic] == qlo)
    if qflags is not None:
        found &= (qflags & 1) != 0
    out[found] = tc[ic[found]] if tc is not None else 1
    return out
