// kmx_count_link_support.hip -- which links of the compacted graph the reads walk (kmx_count_link_support), and an adjacency with
// the bits of chosen links cleared (kmx_count_adjacency_cut).  kmx.h has both rules; they are defined on the arrays alone, so every
// index below is compared with its bound before it is used and any bytes give the answer the rules state.  Indices only: no key
// width here.
//
// Support.  A lane per segment s (grid stride) looks at the pair (s, s + 1): two 32-byte records, neighbouring lanes neighbouring
// records.  Most pairs of a real batch end there -- another read, or a gap.  A junction then gathers: the two offsets of each of its
// unitigs, the two link offsets of t and of mirror(t'), at most four targets of each list -- as in for_links what hides the chain is
// the number of lanes in flight; nothing is staged.  A crossing adds 1 to the slot and, where the mirror link has a slot of its own,
// to that: two 64-bit atomic adds whose result nobody reads.  The three summary counters stay in a register of the lane over its
// stride, are summed over the wave by shuffles and cost one atomic add per wave and counter.  Integer sums only: the result does not
// depend on the order of the atomics, so repeated calls give identical bytes.  No LDS, no scratch.
//
// Cut.  The edges are copied; then a lane per oriented unitig re-derives its links with the function the link kernels run
// (for_links, kmx_count_links.h), so that slot link_offsets[t] + d is the same link here as there, and clears the bit of every slot
// whose cut byte is set.  The two orientations of a one-node unitig own the two nibbles of one byte and four entries share a dword, so
// a bit is cleared by an atomic AND on the aligned dword that holds the byte: the bytes of other entries -- and, at the two ends of an
// array that is not dword-aligned, up to three bytes outside it -- are ANDed with ones and keep their value.  The bits are re-derived
// from the input edges, which the kernel never writes: the result does not depend on the order either.
#include "kmx_device.h"
#include "kmx_launch.h"
#include "kmx_count_links.h"

namespace kmx {

namespace {

constexpr u32 LS_CT = 256;   // threads per block

// two sweeps of a device that holds 2048 lanes on each of 256 compute units: a batch beyond it strides
constexpr u64 LS_MAX_BLOCKS = 4096;

struct SupportIn {
    const u64* segments;
    u64 n_segments;
    const u64* offsets;
    u64 n_unitigs;
    const u64 *link_offsets, *links;
    u64 n_links;
};

__device__ __forceinline__ u64 nodes_of(const SupportIn& in, u64 u) {   // m(u), u < U
    const u64 a = in.offsets[u], b = in.offsets[u + 1u];
    return b >= a ? b - a : 0u;
}

// the first slot of L(t) whose target is `want`, NONE if there is none; t < 2 U.  L(t) is empty unless its slots lie in the array and
// are at most four
constexpr u64 NO_SLOT = ~0ull;
__device__ __forceinline__ u64 slot_of(const SupportIn& in, u64 t, u64 want) {
    const u64 lo = in.link_offsets[t], hi = in.link_offsets[t + 1u];
    const bool fits = (lo <= hi) & (hi <= in.n_links) & (hi - lo <= 4u);
    const u32 n = fits ? (u32)(hi - lo) : 0u;
    u64 slot = NO_SLOT;
#pragma unroll
    for (u32 c = 4u; c-- > 0u;)
        if (c < n && in.links[lo + c] == want) slot = lo + c;
    return slot;
}

__device__ __forceinline__ u32 wave_total(u32 v) {
#pragma unroll
    for (u32 o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void __launch_bounds__(LS_CT) link_support_kernel(SupportIn in, unsigned long long* support, unsigned long long* summary) {
    u32 n_crossed = 0, n_unlinked = 0;   // (a lane sees at most 2^20 pairs: n_segments <= 2^40, and a batch that strides has 2^20 lanes)
    for (u64 s = (u64)blockIdx.x * LS_CT + threadIdx.x; s + 1u < in.n_segments; s += (u64)gridDim.x * LS_CT) {
        const u64* r = in.segments + KMX_PATH_WORDS * s;
        const u64 read = r[KMX_PATH_READ], span = r[KMX_PATH_SPAN], u = r[KMX_PATH_UNITIG], pos = r[KMX_PATH_POS];
        const u64 read2 = r[4u + KMX_PATH_READ], span2 = r[4u + KMX_PATH_SPAN], u2 = r[4u + KMX_PATH_UNITIG], pos2 = r[4u + KMX_PATH_POS];
        const u64 length = span >> 32;
        if (read != read2 || (span2 & 0xFFFFFFFFull) != (span & 0xFFFFFFFFull) + length) continue;   // no junction
        u64 l = NO_SLOT, t = 0, t2 = 0;
        if (u < in.n_unitigs && u2 < in.n_unitigs) {
            const u64 q = pos >> 1, q2 = pos2 >> 1;
            const bool d = (pos & 1u) != 0u, d2 = (pos2 & 1u) != 0u;
            const bool leaves = d ? q + 1u == length : q + length == nodes_of(in, u);   // s ends on the exit node of t
            const bool enters = d2 ? q2 + 1u == nodes_of(in, u2) : q2 == 0u;             // s + 1 starts on the entry node of t'
            t = 2u * u + (d ? 1u : 0u);
            t2 = 2u * u2 + (d2 ? 1u : 0u);
            if (leaves && enters) l = slot_of(in, t, t2);
        }
        if (l == NO_SLOT) {
            ++n_unlinked;
            continue;
        }
        ++n_crossed;
        atomicAdd(support + l, 1ull);
        const u64 m = slot_of(in, t2 ^ 1u, t ^ 1u);   // the mirror link; a hairpin is its own
        if (m != NO_SLOT && m != l) atomicAdd(support + m, 1ull);
    }
    // (every lane of the block comes here: the loop has no early return)
    const u32 c = wave_total(n_crossed), x = wave_total(n_unlinked);
    if ((threadIdx.x & 63u) == 0u) {
        if (c + x != 0u) atomicAdd(summary + 0, (unsigned long long)c + x);
        if (c != 0u) atomicAdd(summary + 1, (unsigned long long)c);
        if (x != 0u) atomicAdd(summary + 2, (unsigned long long)x);
    }
}

__global__ void __launch_bounds__(LS_CT) adjacency_cut_kernel(LinkIn in, const u64* __restrict__ link_offsets, u64 n_links,
                                                              const uint8_t* __restrict__ cut, uint8_t* edges_out) {
    const u64 n_t = 2u * in.n_unitigs;
    for (u64 t = (u64)blockIdx.x * LS_CT + threadIdx.x; t < n_t; t += (u64)gridDim.x * LS_CT) {
        const u64 at = link_offsets[t];
        (void)for_links(t, in, [&](u32 d, u64, u64 i, u32 o, u32 c) {
            // (at + d < n_links always, for offsets kmx_count_unitig_links scanned from the same inputs; i < n: for_links looked)
            if (at < n_links && d < n_links - at && cut[at + d] != 0u) {
                const uintptr_t byte = reinterpret_cast<uintptr_t>(edges_out + i);
                const u32 bit = 8u * (u32)(byte & 3u) + 4u * o + c;
                atomicAnd(reinterpret_cast<unsigned int*>(byte & ~(uintptr_t)3u), ~(1u << bit));
            }
        });
    }
}

unsigned ls_blocks(u64 lanes) {
    const u64 nb = (lanes + LS_CT - 1u) / LS_CT;
    return (unsigned)(nb < LS_MAX_BLOCKS ? nb : LS_MAX_BLOCKS);
}

}  // namespace

// support[l] += the junctions that cross link slot l or its mirror, summary[0 .. 3) += junctions, crossed, unlinked (n_segments >= 2;
// n_unitigs == 0 reads neither offsets array: every junction is unlinked); asynchronous
hipError_t launch_count_link_support(const u64* segments, u64 n_segments, const u64* offsets, u64 n_unitigs, const u64* link_offsets, const u64* links,
                                     u64 n_links, u64* support, u64* summary, hipStream_t st) {
    const SupportIn in{segments, n_segments, offsets, n_unitigs, link_offsets, links, n_links};
    hipLaunchKernelGGL(link_support_kernel, dim3(ls_blocks(n_segments - 1u)), dim3(LS_CT), 0, st, in, reinterpret_cast<unsigned long long*>(support),
                       reinterpret_cast<unsigned long long*>(summary));
    return hipGetLastError();
}

// edges_out = edges with the bit of every cut link slot cleared (n >= 1; n_unitigs or n_links == 0: the copy alone); asynchronous
hipError_t launch_count_adjacency_cut(const uint8_t* edges, const uint8_t* flips, const u64* nbr, u64 n, const u64* nodes, const u64* offsets,
                                      u64 n_unitigs, const u64* place, const u64* link_offsets, u64 n_links, const uint8_t* cut, uint8_t* edges_out,
                                      hipStream_t st) {
    const hipError_t e = hipMemcpyAsync(edges_out, edges, n, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return e;
    if (n_unitigs == 0 || n_links == 0) return hipSuccess;
    const LinkIn in{edges, flips, nbr, nodes, offsets, place, n, n_unitigs};
    hipLaunchKernelGGL(adjacency_cut_kernel, dim3(ls_blocks(2u * n_unitigs)), dim3(LS_CT), 0, st, in, link_offsets, n_links, cut, edges_out);
    return hipGetLastError();
}

}  // namespace kmx
