// kmx_count_dir.h -- the prefix directory over a count table's keys, shared by the kernels that search a table: kmx_count_query.hip
// (the lookup), kmx_count_graph.hip (the adjacency) and kmx_count_correct.hip (the correction, through table_search below).
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

// The search itself, NQ queries of a lane in lockstep (every step issues NQ independent loads): hit[j] = the index of q[j] in the
// table, ~0 if it is absent, not live or has a bit at or above 2k.  The range starts as the query's bin (DIR) or as [0, n); binary
// steps while some range is longer than LINE keys -- q, if the table holds it, stays inside [lo, hi): keys[mid] <= q keeps [mid, hi),
// q < keys[mid] keeps [lo, mid) (lo < mid < hi, so every step shortens the range) -- then the LINE keys of the range are loaded at once
// and the equal one (keys are distinct) is the answer.  Every index is below n.  The lookup kernel's own loop, for the kernels
// that search from inside other work (kmx_count_correct.hip); lookup_kernel keeps its spelling, so its code object does not move.
template <u32 W, bool DIR, u32 NQ>
__device__ __forceinline__ void table_search(const u64* __restrict__ keys, u64 n, u32 k, u32 p, const u32* __restrict__ dir, const Key<W> (&q)[NQ],
                                             const bool (&live)[NQ], u64 (&hit)[NQ]) {
    using K = Key<W>;
    u64 lo[NQ], hi[NQ];
#pragma unroll
    for (u32 j = 0; j < NQ; ++j) {
        lo[j] = hi[j] = 0u;
        if (!live[j] || q[j].outside(k)) continue;
        if (DIR) {
            const u64 b = bin_of<W>(q[j], k, p);
            const u64 a0 = dir[b], a1 = dir[b + 1u];
            lo[j] = a0 < n ? a0 : n;
            hi[j] = a1 < n ? a1 : n;
            if (hi[j] < lo[j]) hi[j] = lo[j];
        } else {
            hi[j] = n;
        }
    }
    for (;;) {
        bool any = false;
#pragma unroll
        for (u32 j = 0; j < NQ; ++j) any |= hi[j] - lo[j] > LINE;
        if (!any) break;
        K m[NQ];
        u64 mid[NQ];
#pragma unroll
        for (u32 j = 0; j < NQ; ++j) {
            mid[j] = lo[j] + ((hi[j] - lo[j]) >> 1);
            m[j] = q[j];
            if (hi[j] - lo[j] > LINE) m[j] = K::load(keys, mid[j]);
        }
#pragma unroll
        for (u32 j = 0; j < NQ; ++j) {
            if (hi[j] - lo[j] > LINE) {
                if (q[j].less(m[j])) hi[j] = mid[j];
                else lo[j] = mid[j];
            }
        }
    }
#pragma unroll
    for (u32 j = 0; j < NQ; ++j) {
        hit[j] = ~0ull;
#pragma unroll
        for (u32 s = 0; s < LINE; ++s) {
            const u64 i = lo[j] + s;
            if (i < hi[j] && K::load(keys, i).equal(q[j])) hit[j] = i;
        }
    }
}

}  // namespace

}  // namespace kmx
