// kmx_count_links.hip -- the unitigs as a graph (kmx_count_unitig_links), and a table cut down by unitig (kmx_count_unitig_select(2)).
//
// Links.  An ORIENTED UNITIG t = 2 u + s leaves through its exit node v = 2 i + o; every set edge bit of entry i on that side names a
// neighbour j, whose place says which unitig it sits in and whether it is that unitig's first or last node: the link's target
// (kmx.h has the rule).  Indices only: no key width here.  A lane per oriented unitig walks a chain of dependent loads -- offsets,
// node, edge and flip byte, then per set bit the neighbour word, its place and one search of the offsets, whose top levels stay in
// cache -- so what hides the chain is the number of lanes in flight; nothing is staged, no LDS beyond the scan's, no atomics.
//   count    a lane per oriented unitig (grid stride): its degree, 0 .. 4, one byte; the bytes are padded with zeros to whole
//            RANGES of 4096 and always hold a slot for t = 2 U, so that the last offset falls out of the same scan.
//   partial  a block per range: the sum of its degrees (16 bytes per thread, one 16-byte load).
//   scan     the family's scan_single_kernel over the ranges' sums: the first link slot of every range, and the total.
//   offsets  a block per range: block scan of the threads' 16-byte sums behind the range's slot -> d_link_offsets[0 .. 2 U].
//   emit     a lane per oriented unitig re-derives its targets and stores them from its offset on: recomputing costs the same loads
//            again, a temporary would cost 32 bytes per oriented unitig written and read.
// Count and emit run the same function (for_links) over the same inputs, so the emit's slots are the scan's; a store is guarded by
// the total all the same.  Every word is written by exactly one lane and depends on the inputs only: repeated calls give identical
// bytes.
//
// Select.  keep[i] = entry i is placed and the unitig of its position is kept: place, one search of the offsets, the keep byte.
// Behind that mark byte the compaction is the filter's: keep_count_kernel and scan_single_kernel of kmx_count_common.h here, over
// the filter's layout of the work buffer, and the filter's own emit (launch_count_filter_emit, compact_write_kernel<W, 1>).
#include "kmx_count_common.h"
#include "kmx_count_links.h"

namespace kmx {

namespace {

constexpr u32 LINK_RANGE = CT * 16u;   // oriented unitigs per block of the partial / offsets kernels, and per scanned partial

// ---------------------------------------------------------------- the links
// (LinkIn and for_links: kmx_count_links.h, shared with the cut of kmx_count_link_support.hip)
__global__ void __launch_bounds__(CT) link_count_kernel(LinkIn in, u64 n_pad, uint8_t* __restrict__ deg) {
    const u64 n_t = 2u * in.n_unitigs;
    for (u64 t = (u64)blockIdx.x * CT + threadIdx.x; t < n_pad; t += (u64)gridDim.x * CT)
        deg[t] = t < n_t ? (uint8_t)for_links(t, in, [](u32, u64, u64, u32, u32) {}) : (uint8_t)0u;
}

// the sum of four degree bytes (each at most 4)
__device__ __forceinline__ u32 degree_sum(u32 w) { return (w * 0x01010101u) >> 24; }

__global__ void __launch_bounds__(CT) link_partial_kernel(const uint8_t* __restrict__ deg, u64* __restrict__ partial) {
    __shared__ u64 sh[CT];
    const uint4 v = *reinterpret_cast<const uint4*>(deg + (u64)blockIdx.x * LINK_RANGE + (u64)threadIdx.x * 16u);
    u64 tot;
    (void)block_exscan(degree_sum(v.x) + degree_sum(v.y) + degree_sum(v.z) + degree_sum(v.w), sh, &tot);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// link_offsets[t] = the links in front of oriented unitig t, t = 0 .. n_t (the padding behind n_t holds zeros: slot n_t is the total)
__global__ void __launch_bounds__(CT) link_offsets_kernel(const uint8_t* __restrict__ deg, const u64* __restrict__ partial, u64 n_t,
                                                          u64* __restrict__ link_offsets) {
    __shared__ u64 sh[CT];
    const u64 t0 = (u64)blockIdx.x * LINK_RANGE + (u64)threadIdx.x * 16u;
    const uint4 v = *reinterpret_cast<const uint4*>(deg + t0);
    const u32 w[4] = {v.x, v.y, v.z, v.w};
    u64 tot;
    u64 run = partial[blockIdx.x] + block_exscan(degree_sum(v.x) + degree_sum(v.y) + degree_sum(v.z) + degree_sum(v.w), sh, &tot);
#pragma unroll
    for (u32 j = 0; j < 16u; ++j) {
        if (t0 + j <= n_t) link_offsets[t0 + j] = run;
        run += (w[j >> 2] >> (8u * (j & 3u))) & 0xFFu;
    }
}

__global__ void __launch_bounds__(CT) link_emit_kernel(LinkIn in, const u64* __restrict__ link_offsets, u64 n_links, u64* __restrict__ links) {
    const u64 n_t = 2u * in.n_unitigs;
    for (u64 t = (u64)blockIdx.x * CT + threadIdx.x; t < n_t; t += (u64)gridDim.x * CT) {
        const u64 at = link_offsets[t];
        (void)for_links(t, in, [&](u32 d, u64 target, u64, u32, u32) {
            if (at + d < n_links) links[at + d] = target;   // (always, for offsets this call scanned from the same inputs)
        });
    }
}

struct LinkArea {
    uint8_t* deg;
    u64* partial;
    u64 n_ranges, n_pad;
};
LinkArea link_area(void* area, u64 n_unitigs) {
    LinkArea a;
    a.n_ranges = ceil_div(2u * n_unitigs + 1u, LINK_RANGE);
    a.n_pad = a.n_ranges * LINK_RANGE;
    a.deg = static_cast<uint8_t*>(area);
    a.partial = reinterpret_cast<u64*>(static_cast<char*>(area) + align256(a.n_pad));
    return a;
}

unsigned stride_blocks(u64 lanes) {
    const u64 nb = ceil_div(lanes, CT);
    return (unsigned)(nb < (1u << 20) ? nb : (1u << 20));
}

// ---------------------------------------------------------------- the selection
// keep[i] = entry i sits in a unitig u with keep_u[u] != 0, over the whole padded range (the compaction reads whole CHUNKs)
__global__ void __launch_bounds__(CT) select_mark_kernel(const u64* __restrict__ place, u64 n, u64 n_pad, const u64* __restrict__ offsets, u64 n_unitigs,
                                                         const uint8_t* __restrict__ keep_u, uint8_t* __restrict__ keep) {
    const u64 i = (u64)blockIdx.x * CT + threadIdx.x;
    if (i >= n_pad) return;
    bool kp = false;
    if (i < n) {
        const u64 p1 = place[i] >> 3;
        if (p1 != 0u && p1 <= offsets[n_unitigs]) kp = keep_u[last_at_or_below(offsets, n_unitigs, p1 - 1u)] != 0u;
    }
    keep[i] = kp ? 1u : 0u;
}

u64 select_pad(u64 n) { return ceil_div(n, CHUNK) * CHUNK; }   // (the filter's filter_pad)

}  // namespace

// ---------------------------------------------------------------- host side
// the links' working set for n_unitigs unitigs: a degree byte per oriented unitig (whole ranges, with a slot for t = 2 U) and a
// partial sum per range (+ the total)
size_t count_links_bytes(u64 n_unitigs) {
    const u64 r = ceil_div(2u * n_unitigs + 1u, LINK_RANGE);
    return align256(r * LINK_RANGE) + align256(8u * (r + 1u));
}

// counts the links (n_unitigs >= 1); synchronous (one host round trip: how many there are)
hipError_t launch_count_links_count(const uint8_t* edges, const uint8_t* flips, const u64* nbr, u64 n, const u64* nodes, const u64* offsets, u64 n_unitigs,
                                    const u64* place, void* area, unsigned long long* h_pinned, u64* h_links, hipStream_t st) {
    const LinkArea a = link_area(area, n_unitigs);
    const LinkIn in{edges, flips, nbr, nodes, offsets, place, n, n_unitigs};
    hipLaunchKernelGGL(link_count_kernel, dim3(stride_blocks(a.n_pad)), dim3(CT), 0, st, in, a.n_pad, a.deg);
    hipLaunchKernelGGL(link_partial_kernel, dim3((unsigned)a.n_ranges), dim3(CT), 0, st, a.deg, a.partial);
    hipLaunchKernelGGL(scan_single_kernel, dim3(1), dim3(CT), 0, st, a.partial, a.n_ranges, a.partial + a.n_ranges);
    return read_back(h_pinned, a.partial + a.n_ranges, 1u, h_links, st);
}

// after launch_count_links_count on the same arrays; links may be nullptr (the offsets only)
hipError_t launch_count_links_emit(const uint8_t* edges, const uint8_t* flips, const u64* nbr, u64 n, const u64* nodes, const u64* offsets, u64 n_unitigs,
                                   const u64* place, const void* area, u64 n_links, u64* link_offsets, u64* links, hipStream_t st) {
    const LinkArea a = link_area(const_cast<void*>(area), n_unitigs);
    const LinkIn in{edges, flips, nbr, nodes, offsets, place, n, n_unitigs};
    hipLaunchKernelGGL(link_offsets_kernel, dim3((unsigned)a.n_ranges), dim3(CT), 0, st, a.deg, a.partial, 2u * n_unitigs, link_offsets);
    if (links && n_links)
        hipLaunchKernelGGL(link_emit_kernel, dim3(stride_blocks(2u * n_unitigs)), dim3(CT), 0, st, in, link_offsets, n_links, links);
    return hipGetLastError();
}

// marks and counts the entries of kept unitigs (n, n_unitigs >= 1) in an area of count_filter_bytes(n), laid out as the filter's (the
// mark bytes in whole CHUNKs, then the partials): launch_count_filter_emit writes the table from it.  Synchronous (one host round
// trip: how many there are)
hipError_t launch_count_select_mark(const u64* place, u64 n, const u64* offsets, u64 n_unitigs, const uint8_t* keep_u, void* area,
                                    unsigned long long* h_pinned, u64* h_out, hipStream_t st) {
    uint8_t* keep = static_cast<uint8_t*>(area);
    u64* partial = reinterpret_cast<u64*>(static_cast<char*>(area) + align256(select_pad(n)));
    const u64 nb = ceil_div(n, CHUNK);
    hipLaunchKernelGGL(select_mark_kernel, dim3((unsigned)ceil_div(select_pad(n), CT)), dim3(CT), 0, st, place, n, select_pad(n), offsets, n_unitigs, keep_u,
                       keep);
    hipLaunchKernelGGL(keep_count_kernel, dim3((unsigned)nb), dim3(CT), 0, st, keep, partial);
    hipLaunchKernelGGL(scan_single_kernel, dim3(1), dim3(CT), 0, st, partial, nb, partial + nb);
    return read_back(h_pinned, partial + nb, 1u, h_out, st);
}

}  // namespace kmx
