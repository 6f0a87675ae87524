"""Vectorised numpy restatements used by the *_sip13 tests.

* siphash13(words, key0, key1): SipHash-1-3 of each u64's 8 little-endian bytes -- hash_one(&DefaultHasher / RandomState, kmer)
  (hash.rs:4-20), the hash of kmx_hash_words_sip13.  Pinned against the oracle's kmo_siphash13_u64 in tests/test_sip13_host.py.
* bucket_of(h, log2_buckets): the BUILD-DEFINED bucket function of kmx_histogram (include/kmx.h).
* lmers / sliding_minimizers: the 2w-bit l-mers of reads in 2-bit codes and the leftmost minimum-hash l-mer of every k-mer --
  what SeqVecMinimizerIter's monotone deque yields (seq_vector/minimizers.rs:39-141), validated against oracle.seqvec_minimizers.
"""
from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1
_C = (0x736F6D6570736575, 0x646F72616E646F6D, 0x6C7967656E657261, 0x7465646279746573)


def _rotl(x: np.ndarray, b: int) -> np.ndarray:
    return (x << np.uint64(b)) | (x >> np.uint64(64 - b))


def _round(v0, v1, v2, v3):
    v0 = v0 + v1; v1 = _rotl(v1, 13); v1 ^= v0; v0 = _rotl(v0, 32)
    v2 = v2 + v3; v3 = _rotl(v3, 16); v3 ^= v2
    v0 = v0 + v3; v3 = _rotl(v3, 21); v3 ^= v0
    v2 = v2 + v1; v1 = _rotl(v1, 17); v1 ^= v2; v2 = _rotl(v2, 32)
    return v0, v1, v2, v3


def siphash13(words, key0: int = 0, key1: int = 0) -> np.ndarray:
    m = np.ascontiguousarray(words).astype(np.uint64, copy=True)
    with np.errstate(over="ignore"):
        k0, k1 = np.uint64(key0 & M64), np.uint64(key1 & M64)
        v0 = np.full_like(m, k0 ^ np.uint64(_C[0]))
        v1 = np.full_like(m, k1 ^ np.uint64(_C[1]))
        v2 = np.full_like(m, k0 ^ np.uint64(_C[2]))
        v3 = (k1 ^ np.uint64(_C[3])) ^ m
        v0, v1, v2, v3 = _round(v0, v1, v2, v3)
        v0 ^= m
        b = np.uint64(8 << 56)
        v3 ^= b
        v0, v1, v2, v3 = _round(v0, v1, v2, v3)
        v0 ^= b
        v2 ^= np.uint64(0xFF)
        for _ in range(3):
            v0, v1, v2, v3 = _round(v0, v1, v2, v3)
        return v0 ^ v1 ^ v2 ^ v3


def bucket_of(h: np.ndarray, log2_buckets: int) -> np.ndarray:
    if log2_buckets == 0:
        return np.zeros(len(h), np.int64)
    h = np.asarray(h, np.uint64)
    lo = (h & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (h >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        mix = lo * np.uint32(0x9E3779B1) + hi * np.uint32(0x85EBCA6B)
    return (mix >> np.uint32(32 - log2_buckets)).astype(np.int64)


def codes_of(ascii_bytes: np.ndarray) -> np.ndarray:
    """what SeqVector::from packs for each byte: (c >> 1) & 3 in internal order, mapped to A0 C1 G2 T3"""
    i = (np.asarray(ascii_bytes, np.uint8) >> 1) & 3
    return (i ^ (i >> 1)).astype(np.uint64)


def lmers(codes: np.ndarray, w: int) -> np.ndarray:
    """codes: (n, L) 2-bit codes -> (n, L - w + 1) l-mer words, base 0 lowest"""
    n, L = codes.shape
    nl = L - w + 1
    out = np.zeros((n, nl), np.uint64)
    for b in range(w):
        out |= codes[:, b: b + nl] << np.uint64(2 * b)
    return out


def sliding_minimizers(lm: np.ndarray, hashes: np.ndarray, k: int, w: int):
    """(n, NL) l-mers and their hashes -> (words, pos) of shape (n, L - k + 1): the leftmost minimum-hash l-mer of each k-mer"""
    span = k - w + 1
    win = np.lib.stride_tricks.sliding_window_view(hashes, span, axis=1)   # (n, NK, span)
    arg = np.argmin(win, axis=2)                                            # the first of equal minima: the leftmost
    pos = np.arange(win.shape[1])[None, :] + arg
    return np.take_along_axis(lm, pos, axis=1), pos.astype(np.uint32)
