// kmx_count_dir.h -- the prefix directory over a count table's keys, shared by the kernels that search a table: kmx_count_query.hip
// (the lookup) and kmx_count_graph.hip (the adjacency).
//   dir[j] = index of the first key whose top p bits (counted down from bit 2k, as the counter's MSD partition counts them) are >= j,
//   j = 0 .. 2^p; p from n so that a bin holds about LINE keys when keys are evenly spread (count_lookup_dir_bytes, kmx_launch.h).
// Built per call by one streaming pass over the keys (a wave per 64 keys: where the prefix steps from a to b the wave's lanes write
// dir[a + 1 .. b] together, so a run of empty bins -- canonical keys are skewed -- is not one lane's loop).  A search reads dir[j] and
// dir[j + 1] and is confined to that bin; entries are clamped to n before they are used, so the directory of a table that is not
// sorted gives wrong answers, never a wild access.  Internal linkage, like kmx_count_common.h: each user compiles its own copy.
#pragma once
#include "kmx_count_common.h"

namespace kmx {

namespace {

constexpr u32 LINE = 8;          // keys the last step of a search loads at once (one-word keys: a 64-byte line; two-word: 128 bytes)
constexpr u32 DIR_MAX_BITS = 28; // at most 2^28 + 1 directory entries (1 GiB)

// the bin of a key; anything a table should not hold (a bit at or above 2k) lands in the last bin instead of outside the directory
template <u32 W>
__device__ __forceinline__ u64 bin_of(const Key<W>& key, u32 k, u32 p) {
    if (p == 0u) return 0u;
    const u64 last = (1ull << p) - 1ull;
    if (key.outside(k)) return last;
    const u64 j = key.prefix(k, p);
    return j > last ? last : j;
}

// One streaming pass: lane i compares the bin of key i with the bin of key i - 1 (key -1: bin "-1", so dir[0 .. bin(key 0)] = 0;
// behind the last key: bin 2^p, so the tail of the directory = n).  Every entry is written exactly once when keys ascend.
template <u32 W>
__global__ void __launch_bounds__(CT) dir_build_kernel(const u64* __restrict__ keys, u64 n, u32 k, u32 p, u32* __restrict__ dir) {
    const u64 i = (u64)blockIdx.x * CT + threadIdx.x;   // 0 .. n: position n closes the directory
    const u32 lane = threadIdx.x & 63u;
    u64 from = 1u, to = 0u;   // this lane's entries: dir[from .. to] = i
    if (i <= n) {
        to = i < n ? bin_of<W>(Key<W>::load(keys, i), k, p) : (1ull << p);
        from = i == 0u ? 0u : bin_of<W>(Key<W>::load(keys, i - 1u), k, p) + 1u;
    }
    unsigned long long todo = __ballot(from <= to);
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1ull;
        const u64 f = __shfl(from, src), t = __shfl(to, src), v = __shfl(i, src);
        for (u64 j = f + lane; j <= t; j += 64u) dir[j] = (u32)v;
    }
}

}  // namespace

}  // namespace kmx
