// kmx_key_hash.h -- what kmx_sketch.hip and kmx_hll.hip share: the key hash of kmx.h ("the counting sketch", KEY HASH; the
// HyperLogLog registers hash their keys the same way) and the grid of a sweep over (keys, flags).  One definition of each: a table's
// keys land in the same block of a sketch and the same register of an estimator on every call that takes them.  Internal linkage,
// like everything in kmx_count_common.h.
#pragma once
#include "kmx_count_common.h"

namespace kmx {

namespace {

constexpr u64 SK_G = 0x9E3779B97F4A7C15ull;

// the key hash of kmx.h: one definition for both widths, a one-word key being (lo, hi = 0)
template <u32 W> __device__ __forceinline__ u64 key_hash(const Key<W>& q, u64 seed);
template <> __device__ __forceinline__ u64 key_hash<1>(const Key<1>& q, u64 seed) { return fmix64(q.lo ^ fmix64(seed + SK_G)); }
template <> __device__ __forceinline__ u64 key_hash<2>(const Key<2>& q, u64 seed) { return fmix64(q.lo ^ fmix64(q.hi + seed + SK_G)); }

// lanes of a sweep: SKETCH_BLOCKS_PER_CU blocks of CT on every compute unit; more keys than that and a lane takes several
constexpr u32 SKETCH_BLOCKS_PER_CU = 4;
unsigned sweep_blocks(u64 n, int n_cu) {
    const u64 cap = (u64)(n_cu > 0 ? n_cu : 256) * SKETCH_BLOCKS_PER_CU, nb = ceil_div(n, CT);
    return (unsigned)(nb < cap ? nb : cap);
}

}  // namespace

}  // namespace kmx
