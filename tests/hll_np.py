"""Host model of the distinct-key estimator (kmx_hll_*, include/kmx.h), byte for byte: the yardstick of tests/test_gpu_hll.py.

* key_hash: the sketch's (tests/sketch_np.py), one definition; inv_fmix64 and keys_for_hashes: fmix64 is a bijection -- two
  xor-shifts by 33 and two odd multipliers -- so key = inv_fmix64(h) ^ fmix64(seed + G) is THE one-word key that hashes to a chosen
  h.  The tests place keys exactly with it: one per register, every rank, w == 0.
* idx_rank / registers / merge / bins: the update of kmx.h with np.maximum.at -- a maximum commutes and is idempotent, so that IS
  what any order of adds leaves -- the bytewise maximum, and the 64 bins of kmx_hll_stats.
* estimate: Ertl's improved estimator from the bins, in Python floats (doubles), spelled as kmx.h spells it.
* sketch_log2_blocks: the closed form of the sketch sizing.

Keys are uint64 arrays: (n,) one-word, (n, 2) two-word rows (low, high).  numpy only; pinned by tests/test_hll_np.py, which needs
no GPU."""
import math

import numpy as np

from tests.sketch_np import G, M64, fmix64, key_hash

__all__ = ["key_hash", "fmix64", "inv_fmix64", "keys_for_hashes", "idx_rank", "registers", "merge", "bins", "estimate", "tolerance",
           "sketch_log2_blocks"]

INV_C1 = pow(0xFF51AFD7ED558CCD, -1, 1 << 64)
INV_C2 = pow(0xC4CEB9FE1A85EC53, -1, 1 << 64)


def _unshift33(x):
    return x ^ (x >> np.uint64(33))      # (x ^= x >> 33 is its own inverse: 2 * 33 >= 64)


def inv_fmix64(h):
    x = np.asarray(h, np.uint64).copy()
    with np.errstate(over="ignore"):
        x = _unshift33(x)
        x *= np.uint64(INV_C2)
        x = _unshift33(x)
        x *= np.uint64(INV_C1)
        x = _unshift33(x)
    return x


def keys_for_hashes(h, seed=0):
    """the one-word keys whose hash under `seed` is h"""
    with np.errstate(over="ignore"):
        return inv_fmix64(h) ^ fmix64(np.array([seed & M64], np.uint64) + G)[0]


def idx_rank(h, p):
    """(register, rank) of every hash: idx = h >> (64 - p); rank = min(clz64(h << p), 64 - p) + 1"""
    h = np.asarray(h, np.uint64)
    idx = (h >> np.uint64(64 - p)).astype(np.int64)
    with np.errstate(over="ignore"):
        w = h << np.uint64(p)
    # clz64 without floats: the bit length by binary search on shifts
    n = np.zeros(len(w), np.int64)
    x = w.copy()
    for s in (32, 16, 8, 4, 2, 1):
        big = (x >> np.uint64(s)) != 0
        n[big] += s
        x[big] >>= np.uint64(s)
    bit_length = n + (x != 0)
    clz = 64 - bit_length
    return idx, (np.minimum(clz, 64 - p) + 1).astype(np.uint8)


def registers(keys, p, seed=0, flags=None, into=None):
    """the registers after adding the keys (those whose flag has bit 0, with flags) to `into` (zeros without): a new array"""
    keys = np.asarray(keys, np.uint64)
    if flags is not None:
        keys = keys[(np.asarray(flags) & 1) != 0]
    regs = np.zeros(1 << p, np.uint8) if into is None else into.copy()
    if len(keys):
        idx, rank = idx_rank(key_hash(keys, seed), p)
        np.maximum.at(regs, idx, rank)
    return regs


def merge(a, b):
    return np.maximum(a, b)


def bins(regs):
    return np.bincount(regs, minlength=64).astype(np.uint64)


def _sigma(x):
    if x == 1.0:
        return math.inf
    y, z = 1.0, x
    while True:
        x *= x
        z0 = z
        z += x * y
        y += y
        if z == z0:
            return z


def _tau(x):
    if x == 0.0 or x == 1.0:
        return 0.0
    y, z = 1.0, 1.0 - x
    while True:
        x = math.sqrt(x)
        z0 = z
        y /= 2.0
        z -= (1.0 - x) ** 2 * y
        if z == z0:
            return z / 3.0


def estimate(hist, p):
    """Ertl's improved estimator from the bins C[0 .. 65 - p] (kmx.h, ESTIMATE)"""
    c = [int(v) for v in hist]
    m, q = float(1 << p), 64 - p
    assert sum(c[:q + 2]) == 1 << p and not any(c[q + 2:])
    z = m * _tau(1.0 - c[q + 1] / m)
    for j in range(q, 0, -1):
        z = (z + c[j]) / 2.0
    z += m * _sigma(c[0] / m)
    return m * m / (2.0 * math.log(2.0)) / z if z else math.inf


def tolerance(p):
    """the relative error the tests allow an estimate: four times the estimator's asymptotic standard error 1.04 / sqrt(2^p)"""
    return 4.0 * 1.04 / math.sqrt(1 << p)


def sketch_log2_blocks(n_distinct, fill=0.25):
    """the smallest b in 0..32 with 1 - exp(-E / (16 * 2^b)) <= fill, in closed form: 16 * 2^b >= E / -ln(1 - fill)"""
    need = n_distinct / (-math.log1p(-fill)) / 16.0      # (callers keep E off the exact powers of two, where rounding decides)
    return 0 if need <= 1.0 else min(math.ceil(math.log2(need)), 32)
