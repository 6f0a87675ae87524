// kmx_count_clean.hip -- which unitigs of the compacted graph to drop (kmx_count_unitig_clean): short dead ends that lose to a sibling
// by mean count, the weaker branch of a simple bubble, short unitigs with no link at all.  kmx.h has the rule; it is defined on the
// arrays alone, so every index below is compared with its bound before it is used and any bytes give the answer the rule states.
//
// A lane per unitig (grid stride).  What a unitig needs is a chain of dependent gathers -- its two offsets, its three link offsets and
// up to eight targets, then per tip the lists of the nodes it leads into and the offsets and sums of the siblings found there, per
// bubble the four lists that close it and the other branch's words -- so, as in for_links of kmx_count_links.hip, what hides the
// chain is the number of lanes in flight; nothing is staged: no LDS, no atomics, no scratch.  The rejections that need the unitig's
// own words only (circular, longer than every limit, a degree pattern no reason has) come first: most lanes of a real graph end there.
// Each lane writes its own keep byte and its own reason byte and nothing else; both depend on the inputs only, so repeated calls give
// identical bytes.  Indices only: no key width here.
#include "kmx_device.h"
#include "kmx_launch.h"

namespace kmx {

namespace {

constexpr u32 CLEAN_CT = 256;   // threads per block

struct CleanIn {
    const u64* offsets;
    const uint8_t* circular;   // nullptr: none is
    const u64* sums;           // nullptr: S(u) = m(u)
    u64 n_unitigs;
    const u64 *link_offsets, *links;
    u64 n_links;
    u64 tip_max, bubble_max, bubble_diff, island_max;
    u32 tip_num, tip_den;
};

// L(t): links[at .. at + n), n = 0 unless the slots lie in the array, are at most four and every target names an oriented unitig.
// The targets stay in memory and are read again where they are used: a lane that holds four lists of four costs more than the loads.
// Flat on purpose, here and below: every early exit is one more level of divergent control flow and holds a pair of scalar registers,
// and written with early returns the kernel spilled 32 of them; so conditions are gathered into a flag and the loads are guarded one
// by one.
struct List {
    u64 at;
    u32 n;
};

__device__ __forceinline__ List list_between(const CleanIn& in, u64 lo, u64 hi) {
    const bool fits = (lo <= hi) & (hi <= in.n_links) & (hi - lo <= 4u);
    const u32 n = fits ? (u32)(hi - lo) : 0u;
    bool ok = true;
#pragma unroll
    for (u32 c = 0; c < 4u; ++c)
        if (c < n) ok &= in.links[lo + c] < 2u * in.n_unitigs;
    return List{lo, ok ? n : 0u};
}

// element c of a list if it has one, else a word no oriented unitig equals
__device__ __forceinline__ u64 target_or_none(const CleanIn& in, const List& l, u32 c) { return c < l.n ? in.links[l.at + c] : ~0ull; }

// (t < 2 U)
__device__ __forceinline__ List list_of(const CleanIn& in, u64 t) { return list_between(in, in.link_offsets[t], in.link_offsets[t + 1u]); }

// m(u) and S(u) for u < U
struct Weight {
    u64 m, s;
};

__device__ __forceinline__ u64 nodes_between(u64 a, u64 b) { return b >= a ? b - a : 0u; }

__device__ __forceinline__ Weight weight_of(const CleanIn& in, u64 u) {
    const u64 m = nodes_between(in.offsets[u], in.offsets[u + 1u]);
    return Weight{m, in.sums ? in.sums[u] : m};
}

// s * m * c, c < 2^16, as three 64-bit limbs: exact for any s and m
struct U192 {
    u64 w0, w1, w2;
};

__device__ __forceinline__ U192 product(u64 s, u64 m, u32 c) {
    const u64 lo = s * m, hi = __umul64hi(s, m);
    const u64 t = hi * c, w1 = t + __umul64hi(lo, (u64)c);
    return U192{lo * c, w1, __umul64hi(hi, (u64)c) + (w1 < t ? 1u : 0u)};
}

// u LOSES to y at (a, b): S(u) m(y) b < S(y) m(u) a, or both sides equal and u > y
__device__ __forceinline__ bool loses(const Weight& wu, u64 u, const Weight& wy, u64 y, u32 a, u32 b) {
    const U192 l = product(wu.s, wy.m, b), r = product(wy.s, wu.m, a);
    const bool low = l.w0 != r.w0 ? l.w0 < r.w0 : u > y;
    const bool mid = l.w1 != r.w1 ? l.w1 < r.w1 : low;
    return l.w2 != r.w2 ? l.w2 < r.w2 : mid;
}

// a dead end that leaves through the list lt: does some sibling at a node it leads into win?
__device__ __forceinline__ bool tip_loses(const CleanIn& in, u64 u, const Weight& wu, const List& lt) {
    bool drop = false;
    for (u32 c = 0; c < lt.n; ++c) {
        const List lx = list_of(in, in.links[lt.at + c] ^ 1u);   // the mirrors of everything that enters x
        for (u32 e = 0; e < lx.n; ++e) {
            const u64 yu = in.links[lx.at + e] >> 1;
            const bool lost = loses(wu, u, weight_of(in, yu), yu, in.tip_num, in.tip_den);
            drop |= (yu != u) & lost;
        }
    }
    return drop;
}

// d0 = d1 = 1: is u the losing branch of a simple bubble from s to x?  (x, s < 2 U)
__device__ __forceinline__ bool bubble_loses(const CleanIn& in, u64 u, const Weight& wu, u64 x, u64 s) {
    const List ls = list_of(in, s);
    const u64 s0 = target_or_none(in, ls, 0u), s1 = target_or_none(in, ls, 1u);
    if (!((ls.n == 2u) & (s0 != s1) & ((s0 == 2u * u) | (s1 == 2u * u)))) return false;   // (most lanes that came this far leave here)
    const u64 y = s0 == 2u * u ? s1 : s0, yu = y >> 1, mu = 2u * u + 1u, my = y ^ 1u;
    const List lx = list_of(in, x ^ 1u), ly = list_of(in, y), lm = list_of(in, my);
    const u64 x0 = target_or_none(in, lx, 0u), x1 = target_or_none(in, lx, 1u);
    bool ok = (lx.n == 2u) & (((x0 == mu) & (x1 == my)) | ((x0 == my) & (x1 == mu)));
    const u64 y0 = target_or_none(in, ly, 0u), m0 = target_or_none(in, lm, 0u);
    ok &= (ly.n == 1u) & (y0 == x) & (lm.n == 1u) & (m0 == (s ^ 1u));
    ok &= (u != yu) & (u != s >> 1) & (u != x >> 1) & (yu != s >> 1) & (yu != x >> 1);
    const Weight wy = weight_of(in, yu);
    ok &= !(in.circular && in.circular[yu] != 0u);
    ok &= (wy.m <= in.bubble_max) & ((wu.m > wy.m ? wu.m - wy.m : wy.m - wu.m) <= in.bubble_diff);
    const bool lost = loses(wu, u, wy, yu, 1u, 1u);
    return ok & lost;
}

__global__ void __launch_bounds__(CLEAN_CT) unitig_clean_kernel(CleanIn in, uint8_t* __restrict__ keep, uint8_t* __restrict__ reason) {
    const u64 longest = max(in.tip_max, max(in.bubble_max, in.island_max));
    for (u64 u = (u64)blockIdx.x * CLEAN_CT + threadIdx.x; u < in.n_unitigs; u += (u64)gridDim.x * CLEAN_CT) {
        u32 why = KMX_CLEAN_KEEP;
        const u64 m = nodes_between(in.offsets[u], in.offsets[u + 1u]);
        if (m <= longest && !(in.circular && in.circular[u] != 0u)) {
            const u64 l0 = in.link_offsets[2u * u], l1 = in.link_offsets[2u * u + 1u], l2 = in.link_offsets[2u * u + 2u];
            const List a = list_between(in, l0, l1), b = list_between(in, l1, l2);
            if (a.n == 0u && b.n == 0u) {
                if (in.island_max != 0u && m <= in.island_max) why = KMX_CLEAN_ISLAND;
            } else if (a.n == 0u || b.n == 0u) {
                if (in.tip_max != 0u && m <= in.tip_max &&
                    (in.tip_num == 0u || tip_loses(in, u, Weight{m, in.sums ? in.sums[u] : m}, a.n ? a : b)))
                    why = KMX_CLEAN_TIP;
            } else if (a.n == 1u && b.n == 1u) {
                if (in.bubble_max != 0u && m <= in.bubble_max &&
                    bubble_loses(in, u, Weight{m, in.sums ? in.sums[u] : m}, in.links[a.at], in.links[b.at] ^ 1u))
                    why = KMX_CLEAN_BUBBLE;
            }
        }
        keep[u] = why == KMX_CLEAN_KEEP ? 1u : 0u;
        if (reason) reason[u] = (uint8_t)why;
    }
}

// two sweeps of a device that holds 2048 lanes on each of 256 compute units: a graph beyond it strides
constexpr u64 CLEAN_MAX_BLOCKS = 4096;

}  // namespace

// one keep byte per unitig (n_unitigs >= 1) and, unless reason == nullptr, one reason byte; circular and sums may be nullptr; asynchronous
hipError_t launch_count_unitig_clean(const u64* offsets, const uint8_t* circular, const u64* sums, u64 n_unitigs, const u64* link_offsets,
                                     const u64* links, u64 n_links, u64 tip_max, u32 tip_num, u32 tip_den, u64 bubble_max, u64 bubble_diff,
                                     u64 island_max, uint8_t* keep, uint8_t* reason, hipStream_t st) {
    const CleanIn in{offsets, circular, sums, n_unitigs, link_offsets, links, n_links, tip_max, bubble_max, bubble_diff, island_max, tip_num, tip_den};
    const u64 nb = (n_unitigs + CLEAN_CT - 1u) / CLEAN_CT;
    hipLaunchKernelGGL(unitig_clean_kernel, dim3((unsigned)(nb < CLEAN_MAX_BLOCKS ? nb : CLEAN_MAX_BLOCKS)), dim3(CLEAN_CT), 0, st, in, keep, reason);
    return hipGetLastError();
}

}  // namespace kmx
