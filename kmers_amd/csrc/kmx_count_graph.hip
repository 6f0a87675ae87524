// kmx_count_graph.hip -- a count table read as the node set of a de Bruijn graph: kmx_count_adjacency(2) (which of the eight
// possible neighbours of every entry are in the table), kmx_count_edge_histogram (how often each edge byte occurs) and
// kmx_count_unitig_ends (where the non-branching paths end).
//
// Adjacency.  x = the key of entry i read as the forward strand, r = rc(x).  Edge slot c is the successor S_c(x) = (x >> 2) | c at
// the top base, slot 4 + c the predecessor P_c(x) = ((x << 2) | c) & mask; the node of a neighbouring word w is min(w, rc(w)).  On
// each side the eight spellings are two families of four:
//   group  g | j, j = 0..3, g = (r << 2) & mask on the successor side (rc(S_c) with j = 3 - c) and (x << 2) & mask on the predecessor
//          side (P_c with j = c): four consecutive integers -- ONE lower bound of g, then the keys behind it, settles all four;
//   far    f with top base 3 - j, f = x >> 2 (S_c, c = 3 - j) and r >> 2 (rc(P_c), c = j): they differ in their top base and lie far
//          apart, a search each.
// min(group, far) is decided BEFORE anything is searched: a far word is searched only where it is the smaller spelling (its top base
// is below the group's: about every second one), the group only where it wins for some j.  So a lane runs at most ten searches -- two
// groups, eight far words, typically five -- in lockstep: every step issues its loads independently, as lookup_kernel does.  A search
// is a lower bound: binary steps while the range is longer than ADJ_LEAF keys, then the keys from `lo` on are loaded at once (five
// cover the lower bound of a far word, eight the four keys of a group) and compared.  With the directory of kmx_count_lookup
// (kmx_count_dir.h) the range starts as the word's bin, without it as [0, n).  Counts are read only where presence depends on them
// and a key was hit.  Loads past the range are bounded by n, and directory entries are clamped to n: a table that is not sorted
// gives wrong answers, never a wild access.  Vector loads and stores only; no LDS, no atomics, no scratch.
//
// Edge histogram.  Bins per wave in LDS (u32: a wave sees fewer than 2^32 bytes), 16 bytes per lane and step where the array is
// 16-byte aligned, the bytes before and behind that by block 0; one device atomic per non-empty bin and block.
//
// Unitig ends.  A lane per entry: its edge byte, and for a side with one edge the edge byte of that one neighbour.
#include "kmx_count_dir.h"

namespace kmx {

namespace {

constexpr u32 ADJ_FAR = 8;                // far searches of a lane: slot 4 * side + j
constexpr u32 ADJ_NS = ADJ_FAR + 2;       // ... and the two groups behind them
constexpr u32 ADJ_LEAF = 4;               // binary steps stop at a range of this many keys: the lower bound is one of lo .. lo + ADJ_LEAF
constexpr u32 ADJ_GROUP = ADJ_LEAF + 4;   // keys loaded for a group: its four keys start at the lower bound
constexpr u64 NO_ENTRY = ~0ull;           // KMX_NO_ENTRY
constexpr u32 EH_VEC = 16;                // bytes per lane and step of the edge histogram

// ---------------------------------------------------------------- the adjacency
// EXTRA: flips and / or neighbour indices are asked for (each may still be nullptr); without it the edge bytes alone.
template <u32 W, bool DIR, bool EXTRA>
__global__ void __launch_bounds__(CT) adjacency_kernel(const u64* __restrict__ keys, const u64* __restrict__ counts, u64 n, u32 k, u32 p,
                                                       const u32* __restrict__ dir, u64 min_count, uint8_t* __restrict__ edges,
                                                       uint8_t* __restrict__ flips, u64* __restrict__ nbr) {
    using K = Key<W>;
    const bool by_count = counts != nullptr && min_count != 0u;   // (every u64 is >= 0)
    for (u64 i = (u64)blockIdx.x * CT + threadIdx.x; i < n; i += (u64)gridDim.x * CT) {
        const K x = K::load(keys, i);
        bool present = !x.outside(k);
        if (present && by_count) present = counts[i] >= min_count;
        K q[ADJ_NS];
        u64 lo[ADJ_NS], hi[ADJ_NS];
        u32 live = 0u, group = 0u, flip = 0u;   // bit 4 * side + j (live: and bits 8, 9 for the groups)
        const K r = x.revcomp(k);
#pragma unroll
        for (u32 s = 0; s < 2u; ++s) {
            const K g = (s == 0u ? r : x).shl_base(k), f = (s == 0u ? x : r).shr_base();
#pragma unroll
            for (u32 j = 0; j < 4u; ++j) {
                const u32 b = 4u * s + j;
                const K gw = g.with_low(2u, j), fw = f.with_top(k, 3u - j);
                const bool far = fw.less(gw);
                q[b] = fw;
                if (far) live |= 1u << b;
                else group |= 1u << b;
                // the word as spelled on x's strand is the far one on the successor side, the group one on the predecessor side
                if (s == 0u ? gw.less(fw) : far) flip |= 1u << b;
            }
            q[ADJ_FAR + s] = g;
            if ((group >> (4u * s)) & 15u) live |= 1u << (ADJ_FAR + s);
        }
        if (!present) live = 0u;
#pragma unroll
        for (u32 s = 0; s < ADJ_NS; ++s) {
            lo[s] = hi[s] = 0u;
            if (!((live >> s) & 1u)) continue;
            if (DIR) {
                const u64 b = bin_of<W>(q[s], k, p);
                const u64 a0 = dir[b], a1 = dir[b + 1u];
                lo[s] = a0 < n ? a0 : n;
                hi[s] = a1 < n ? a1 : n;
                if (hi[s] < lo[s]) hi[s] = lo[s];
            } else {
                hi[s] = n;
            }
        }
        // lower bound of q in [lo, hi]: keys[mid] < q keeps (mid, hi], otherwise [lo, mid] (lo <= mid < hi: every step shortens)
        for (;;) {
            bool any = false;
#pragma unroll
            for (u32 s = 0; s < ADJ_NS; ++s) any |= hi[s] - lo[s] > ADJ_LEAF;
            if (!any) break;
            K m[ADJ_NS];
            u64 mid[ADJ_NS];
#pragma unroll
            for (u32 s = 0; s < ADJ_NS; ++s) {
                mid[s] = lo[s] + ((hi[s] - lo[s]) >> 1);
                m[s] = q[s];
                if (hi[s] - lo[s] > ADJ_LEAF) m[s] = K::load(keys, mid[s]);
            }
#pragma unroll
            for (u32 s = 0; s < ADJ_NS; ++s) {
                if (hi[s] - lo[s] > ADJ_LEAF) {
                    if (m[s].less(q[s])) lo[s] = mid[s] + 1u;
                    else hi[s] = mid[s];
                }
            }
        }
        // the lower bound is one of lo .. lo + ADJ_LEAF: a far word is the key there or nowhere, a group's keys are the four from there
        u64 nb[ADJ_FAR];
#pragma unroll
        for (u32 s = 0; s < ADJ_FAR; ++s) {
            nb[s] = NO_ENTRY;
#pragma unroll
            for (u32 t = 0; t <= ADJ_LEAF; ++t) {
                const u64 e = lo[s] + t;
                if (((live >> s) & 1u) && e < n && K::load(keys, e).equal(q[s])) nb[s] = e;
            }
        }
#pragma unroll
        for (u32 s = 0; s < 2u; ++s) {
#pragma unroll
            for (u32 t = 0; t < ADJ_GROUP; ++t) {
                const u64 e = lo[ADJ_FAR + s] + t;
                if (!((live >> (ADJ_FAR + s)) & 1u) || e >= n) continue;
                const K v = K::load(keys, e);
                if (!v.with_low(2u, 0u).equal(q[ADJ_FAR + s])) continue;
#pragma unroll
                for (u32 j = 0; j < 4u; ++j)
                    if ((v.bits(0u) & 3u) == j && ((group >> (4u * s + j)) & 1u)) nb[4u * s + j] = e;
            }
        }
        if (by_count) {   // a neighbour that is not present is no neighbour
            u64 c[ADJ_FAR];
#pragma unroll
            for (u32 s = 0; s < ADJ_FAR; ++s) c[s] = nb[s] != NO_ENTRY ? counts[nb[s]] : 0u;
#pragma unroll
            for (u32 s = 0; s < ADJ_FAR; ++s)
                if (c[s] < min_count) nb[s] = NO_ENTRY;
        }
        // slot of bit 4 * side + j: the successor side spells c = 3 - j, the predecessor side c = j
        u32 eb = 0u, fb = 0u;
#pragma unroll
        for (u32 b = 0; b < ADJ_FAR; ++b) {
            const u32 e = b < 4u ? 3u - b : b;
            if (nb[b] != NO_ENTRY) {
                eb |= 1u << e;
                fb |= ((flip >> b) & 1u) << e;
            }
            if (EXTRA && nbr != nullptr) nbr[8u * i + e] = nb[b];
        }
        edges[i] = (uint8_t)eb;
        if (EXTRA && flips != nullptr) flips[i] = (uint8_t)fb;
    }
}

// ---------------------------------------------------------------- the edge histogram
__global__ void __launch_bounds__(CT) edge_hist_kernel(const uint8_t* __restrict__ edges, u64 n, unsigned long long* __restrict__ hist) {
    __shared__ u32 bins[CT / 64u][256];
    for (u32 b = threadIdx.x; b < (CT / 64u) * 256u; b += CT) (&bins[0][0])[b] = 0u;
    __syncthreads();
    u32* mine = bins[threadIdx.x >> 6];
    u64 head = (EH_VEC - (u32)(reinterpret_cast<uintptr_t>(edges) & (EH_VEC - 1u))) & (EH_VEC - 1u);   // bytes before the aligned part
    if (head > n) head = n;
    const u64 n_vec = (n - head) / EH_VEC;
    const uint4* vec = reinterpret_cast<const uint4*>(edges + head);
    for (u64 t = (u64)blockIdx.x * CT + threadIdx.x; t < n_vec; t += (u64)gridDim.x * CT) {
        const uint4 v = vec[t];
        const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (u32 j = 0; j < 4u; ++j) {
#pragma unroll
            for (u32 b = 0; b < 4u; ++b) atomicAdd(&mine[(w[j] >> (8u * b)) & 255u], 1u);
        }
    }
    if (blockIdx.x == 0) {   // the bytes before and behind the aligned part: fewer than 2 * EH_VEC
        const u64 tail_at = head + n_vec * EH_VEC, rest = head + (n - tail_at);
        for (u64 t = threadIdx.x; t < rest; t += CT) atomicAdd(&mine[edges[t < head ? t : tail_at + (t - head)]], 1u);
    }
    __syncthreads();
    for (u32 b = threadIdx.x; b < 256u; b += CT) {
        u64 v = 0u;
#pragma unroll
        for (u32 w = 0; w < CT / 64u; ++w) v += bins[w][b];
        if (v != 0u) atomicAdd(&hist[b], (unsigned long long)v);
    }
}

// ---------------------------------------------------------------- the unitig ends
// Is side `s` (0: successors, the low nibble; 1: predecessors, the high nibble) of entry i the end of a non-branching path?
__device__ __forceinline__ bool side_ends(const uint8_t* __restrict__ edges, const u64* __restrict__ nbr, u64 n, u64 i, u32 eb, u32 fb, u32 s) {
    const u32 nib = (eb >> (4u * s)) & 15u;
    if (__popc(nib) != 1) return true;
    const u32 e = 4u * s + (u32)__ffs((int)nib) - 1u;
    const u64 j = nbr[8u * i + e];
    if (j >= n || j == i) return true;   // (an index outside the table: inconsistent inputs, nothing is read there)
    // a successor edge enters its neighbour at the predecessor side, a predecessor edge at the successor side; a flipped one at the other
    const bool high = (s == 0u) != (((fb >> e) & 1u) != 0u);
    const u32 other = edges[j];
    return __popc(high ? other >> 4 : other & 15u) != 1;
}

__global__ void __launch_bounds__(CT) unitig_ends_kernel(const uint8_t* __restrict__ edges, const uint8_t* __restrict__ flips,
                                                         const u64* __restrict__ nbr, u64 n, uint8_t* __restrict__ ends) {
    for (u64 i = (u64)blockIdx.x * CT + threadIdx.x; i < n; i += (u64)gridDim.x * CT) {
        const u32 eb = edges[i], fb = flips[i];
        const u32 e0 = side_ends(edges, nbr, n, i, eb, fb, 0u) ? 1u : 0u, e1 = side_ends(edges, nbr, n, i, eb, fb, 1u) ? 2u : 0u;
        ends[i] = (uint8_t)(e0 | e1);
    }
}

// a lane per entry; above 2^30 blocks the lanes loop
unsigned entry_grid(u64 n) {
    const u64 nb = ceil_div(n, CT);
    return (unsigned)(nb < (1ull << 30) ? nb : (1ull << 30));
}

}  // namespace

// ---------------------------------------------------------------- host side
// dir_area: room for the directory of count_lookup_dir_bytes(n, k, &p), or nullptr = the plain search
hipError_t launch_count_adjacency(u32 words, const u64* keys, const u64* counts, u64 n, u32 k, u64 min_count, uint8_t* edges, uint8_t* flips,
                                  u64* nbr, void* dir_area, u32 p, hipStream_t st) {
    u32* dir = static_cast<u32*>(dir_area);
    const bool extra = flips != nullptr || nbr != nullptr;
    const dim3 grid(entry_grid(n)), block(CT);
    with_width(words, [&](auto w) {
        constexpr u32 W = decltype(w)::value;
        if (dir) hipLaunchKernelGGL(dir_build_kernel<W>, dim3((unsigned)ceil_div(n + 1u, CT)), block, 0, st, keys, n, k, p, dir);
        if (dir && extra) hipLaunchKernelGGL((adjacency_kernel<W, true, true>), grid, block, 0, st, keys, counts, n, k, p, dir, min_count, edges, flips, nbr);
        else if (dir) hipLaunchKernelGGL((adjacency_kernel<W, true, false>), grid, block, 0, st, keys, counts, n, k, p, dir, min_count, edges, flips, nbr);
        else if (extra) hipLaunchKernelGGL((adjacency_kernel<W, false, true>), grid, block, 0, st, keys, counts, n, k, p, dir, min_count, edges, flips, nbr);
        else hipLaunchKernelGGL((adjacency_kernel<W, false, false>), grid, block, 0, st, keys, counts, n, k, p, dir, min_count, edges, flips, nbr);
    });
    return hipGetLastError();
}

hipError_t launch_count_edge_histogram(const uint8_t* edges, u64 n, u64* hist, int n_cu, hipStream_t st) {
    u64 nb = ceil_div(n, (u64)CT * EH_VEC);
    const u64 cap = (u64)(n_cu > 128 ? n_cu : 128) * 8u;   // (at least 1024 blocks at 2^40 entries: a wave's u32 bins hold what it sees)
    if (nb > cap) nb = cap;
    hipLaunchKernelGGL(edge_hist_kernel, dim3((unsigned)nb), dim3(CT), 0, st, edges, n, reinterpret_cast<unsigned long long*>(hist));
    return hipGetLastError();
}

hipError_t launch_count_unitig_ends(const uint8_t* edges, const uint8_t* flips, const u64* nbr, u64 n, uint8_t* ends, hipStream_t st) {
    hipLaunchKernelGGL(unitig_ends_kernel, dim3(entry_grid(n)), dim3(CT), 0, st, edges, flips, nbr, n, ends);
    return hipGetLastError();
}

}  // namespace kmx
