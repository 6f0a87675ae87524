"""Host model of the counting sketch (kmx_sketch_*, include/kmx.h), bit for bit: the yardstick of tests/test_gpu_sketch.py.

* fmix64, key_hash, cells_of: the murmur3 finaliser, the key hash (one definition for one- and two-word keys) and the four byte
  offsets of a key's cells.
* new / add / estimate / merge / stats: the sketch as a uint8 array.  add sums the weights into a wide array with np.add.at and
  clips once: saturating adds commute, so that IS what any order of adds leaves.
* min_mask / table_min: the filter of kmx_count_canonical_min(2) as a mask on the windows ahead of count_np.table_of.
* count_solid: the two passes of Context.count_solid over batches of (canon, flags).
* solid_batches: the read batches of the end-to-end cases -- ragged reads drawn from one small genome with substitutions.

Keys are uint64 arrays: (n,) one-word, (n, 2) two-word rows (low, high).  numpy only; pinned by tests/test_sketch_np.py, which
needs no GPU."""
import numpy as np

from tests.count_np import table_of

M64 = (1 << 64) - 1
G = np.uint64(0x9E3779B97F4A7C15)


def fmix64(x):
    x = np.asarray(x, np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
    return x


def key_hash(keys, seed=0):
    keys = np.asarray(keys, np.uint64)
    lo, hi = (keys, np.zeros(len(keys), np.uint64)) if keys.ndim == 1 else (keys[:, 0], keys[:, 1])
    with np.errstate(over="ignore"):
        return fmix64(lo ^ fmix64(hi + np.uint64(seed & M64) + G))


def cells_of(keys, log2_blocks, seed=0):
    """(n, 4) int64: the byte offsets of the cells of every key, row by row"""
    h = key_hash(keys, seed)
    block = (h >> np.uint64(64 - log2_blocks)) if log2_blocks else np.zeros(len(h), np.uint64)
    cols = [np.uint64(64) * block + np.uint64(16 * j) + ((h >> np.uint64(4 * j)) & np.uint64(15)) for j in range(4)]
    return np.stack(cols, axis=1).astype(np.int64)


def new(log2_blocks):
    return np.zeros(64 << log2_blocks, np.uint8)


def add(sketch, keys, log2_blocks, seed=0, weights=None, flags=None):
    """the sketch after adding the keys (those whose flag has bit 0, with flags) with their weights (1 each without): a new array"""
    keys = np.asarray(keys, np.uint64)
    w = np.ones(len(keys), np.uint64) if weights is None else np.minimum(np.asarray(weights, np.uint64), np.uint64(255))
    if flags is not None:
        live = (np.asarray(flags) & 1) != 0
        keys, w = keys[live], w[live]
    wide = sketch.astype(np.uint64)
    if len(keys):
        np.add.at(wide, cells_of(keys, log2_blocks, seed).ravel(), np.repeat(w, 4))
    return np.minimum(wide, 255).astype(np.uint8)


def estimate(sketch, keys, log2_blocks, seed=0, flags=None):
    keys = np.asarray(keys, np.uint64)
    if len(keys) == 0:
        return np.zeros(0, np.uint8)
    est = sketch[cells_of(keys, log2_blocks, seed)].min(axis=1)
    if flags is not None:
        est = np.where((np.asarray(flags) & 1) != 0, est, 0).astype(np.uint8)
    return est


def merge(a, b):
    return np.minimum(a.astype(np.uint16) + b.astype(np.uint16), 255).astype(np.uint8)


def stats(sketch):
    return np.bincount(sketch, minlength=256).astype(np.uint64)


def fill(sketch):
    return float(np.count_nonzero(sketch)) / len(sketch)


def min_mask(sketch, canon, flags, log2_blocks, seed, min_est):
    """the flags kmx_count_canonical_min(2) sorts: bit 0 cleared where the estimate is below min_est"""
    flags = np.asarray(flags, np.uint8)
    if min_est > 255:
        return flags & np.uint8(0xFE)
    keep = estimate(sketch, canon, log2_blocks, seed).astype(np.int64) >= min_est
    return np.where(keep, flags, flags & np.uint8(0xFE)).astype(np.uint8)


def table_min(sketch, canon, flags, log2_blocks, seed, min_est):
    return table_of(canon, min_mask(sketch, canon, flags, log2_blocks, seed, min_est))


def _merge_tables(ka, ca, kb, cb):
    """the union of two tables, counts of equal keys added"""
    keys = np.concatenate([ka, kb])
    cnts = np.concatenate([ca, cb]).astype(np.uint64)
    if len(keys) == 0:
        return keys, cnts
    if keys.ndim == 1:
        u, inv = np.unique(keys, return_inverse=True)
    else:
        order = np.lexsort((keys[:, 0], keys[:, 1]))
        keys, cnts = keys[order], cnts[order]
        head = np.ones(len(keys), bool)
        head[1:] = (keys[1:] != keys[:-1]).any(axis=1)
        u, inv = keys[head], np.cumsum(head) - 1
    out = np.zeros(len(u), np.uint64)
    np.add.at(out, inv.ravel(), cnts)
    return u, out


def count_solid(batches, min_count, log2_blocks, seed=0):
    """Context.count_solid over batches of (canon, flags) -> (kmers, counts, sketch, the size of every batch's table)"""
    first = np.asarray(batches[0][0], np.uint64)
    sk = new(log2_blocks)
    for canon, flags in batches:
        sk = add(sk, canon, log2_blocks, seed, flags=flags)
    keys, cnts, sizes = first[:0], np.zeros(0, np.uint64), []
    for canon, flags in batches:
        bk, bc = table_min(sk, np.asarray(canon, np.uint64), flags, log2_blocks, seed, min_count)
        sizes.append(len(bc))
        keys, cnts = _merge_tables(keys, cnts, bk, bc)
    keep = cnts >= min_count
    return keys[keep], cnts[keep], sk, sizes


def solid_batches(seed, genome_len=100_000, n_batches=4, n_reads=2000, max_len=160, sub_rate=0.01):
    """[(bases uint8, offsets uint64[n_reads + 1])]: n_batches ragged batches of n_reads reads of 40..max_len bases from either
    strand of one random genome -- about 8x coverage as a whole at the defaults -- every base substituted with probability sub_rate:
    most distinct k-mers of such data are errors that occur once, the case the sketch is for."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    comp = np.zeros(256, np.uint8)
    comp[acgt] = np.frombuffer(b"TGCA", np.uint8)
    genome = rng.choice(acgt, genome_len).astype(np.uint8)
    out = []
    for _ in range(n_batches):
        lens = rng.integers(40, max_len + 1, n_reads)
        starts = rng.integers(0, genome_len - max_len, n_reads)
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        bases = np.empty(int(offsets[-1]), np.uint8)
        for r in range(n_reads):
            piece = genome[starts[r]:starts[r] + lens[r]]
            if rng.random() < 0.5:
                piece = comp[piece[::-1]]
            bases[int(offsets[r]):int(offsets[r + 1])] = piece
        hit = rng.random(len(bases)) < sub_rate
        bases[hit] = acgt[(np.searchsorted(acgt, bases[hit]) + rng.integers(1, 4, int(hit.sum()))) % 4]
        out.append((bases, offsets))
    return out
