// kmx_count_links.h -- the links of an oriented unitig, re-derived from the adjacency: the one function that kmx_count_links.hip
// (count, emit) and kmx_count_link_support.hip (the cut) run over the same inputs, so that the d-th link of t is the same link -- and
// the same edge bit -- in all three.  Everything here has internal linkage, as in kmx_count_common.h.
#pragma once
#include "kmx_device.h"

namespace kmx {

namespace {

// the largest i in [0, n) with a[i] <= x (0 if there is none); n >= 1; reads a[1 .. n) only (kmx_count_paths.hip has its twin)
__device__ __forceinline__ u64 last_at_or_below(const u64* __restrict__ a, u64 n, u64 x) {
    u64 lo = 0, hi = n;
    while (hi - lo > 1u) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct LinkIn {
    const uint8_t *edges, *flips;
    const u64 *nbr, *nodes, *offsets, *place;
    u64 n, n_unitigs;
};

// emit(d, target, i, o, c) for the d-th link of oriented unitig t (t < 2 n_unitigs), in ascending c: the link was derived from bit
// 4 o + c of the edge byte of entry i, the exit node's (i < n); returns how many there are.  nbr is read under a set edge bit only.
template <typename F>
__device__ __forceinline__ u32 for_links(u64 t, const LinkIn& in, F&& emit) {
    const u64 n_nodes = in.offsets[in.n_unitigs];
    const u64 a = in.offsets[t >> 1], b = in.offsets[(t >> 1) + 1u];
    if (a >= b || b > n_nodes) return 0u;   // (an empty unitig, or offsets that do not ascend)
    const u64 v = (t & 1u) == 0u ? in.nodes[b - 1u] : in.nodes[a] ^ 1u;
    const u64 i = v >> 1;
    if (i >= in.n) return 0u;
    const u32 o = (u32)(v & 1u);
    const u32 eb = ((u32)in.edges[i] >> (4u * o)) & 15u, fb = ((u32)in.flips[i] >> (4u * o)) & 15u;
    u32 d = 0;
#pragma unroll
    for (u32 c = 0; c < 4u; ++c) {
        if ((eb >> c & 1u) == 0u) continue;
        const u64 j = in.nbr[8u * i + 4u * o + c];
        if (j >= in.n) continue;
        const u64 x = in.place[j], p1 = x >> 3;
        if (p1 == 0u || p1 > n_nodes) continue;   // in no unitig, or a position p = p1 - 1 outside the offsets
        const bool same = ((o ^ (fb >> c)) & 1u) == (u32)(x & 1u);   // w enters j as j is written in its unitig
        if ((x & (same ? 2u : 4u)) == 0u) continue;                    // ... then it must be the first node, else the last
        emit(d, 2u * last_at_or_below(in.offsets, in.n_unitigs, p1 - 1u) + (same ? 0u : 1u), i, o, c);
        ++d;
    }
    return d;
}

}  // namespace

}  // namespace kmx
