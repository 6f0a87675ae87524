// kmx_count_components.hip -- which unitigs of the compacted graph hang together (kmx_count_unitig_components): a label per unitig
// (the smallest unitig index of its connected component), the components numbered in ascending order of that root, and a record of
// four words per component.  kmx.h has the rule; it is defined on the arrays alone, so every index below is compared with its bound
// before it is used and any bytes give the answer the rule states.  Indices only: no key width here.
//
// `labels` itself is the parent array of a forest: parent[u] <= u always, and a value only ever goes down, towards the component's
// minimum.  A lane per unitig (grid stride) in every kernel:
//   init     parent[u] = u, or KMX_COMPONENT_NONE for a unitig the mask leaves out.
//   hook     for each of the at most eight valid link targets v of an alive u (v alive, v != u): pu = parent[u], pv = parent[v]; where
//            they differ, a 64-bit atomicMin of the smaller into parent[the larger].
//   jump     parent[u] = parent[parent[u]]: ONE step per launch.  A lane never chases pointers: unitigs numbered along a chromosome
//            form a chain that the first hook turns into a tree of depth U, and the depth goes by doubling over the rounds.
// A ROUND is hook, then jump, then one word read back: the number of waves that saw a difference so far.  The call ends on the first
// round that adds nothing to it: every valid link then joins equal parents and every parent is a root, read after a kernel
// boundary, so every unitig of a component has the same parent r, r is one of them and r <= each: the minimum.
// STALE LOADS.  Within a launch a plain load of parent[] may return an older value than an atomic on another XCD has written since.
// An older value is a value the word held earlier in the same launch, hence >= the current one and still a member of the same
// component: hooking with it is a correct, merely later, move; and a lane that sees a difference counts it, so the call cannot end on
// it.  Progress does not depend on freshness either: the set A of unitigs whose parent is the component's minimum r only grows (r is
// final wherever it stands), and while A is not the whole component some link joins u in A to v outside it: the hook then lowers
// parent[pv] to r, or pv is in A already and the jump brings v in.  At most |component| + 1 rounds, whatever the loads return; the
// host stops with an error beyond U + 2, which no input reaches.
//   roots    a block per RANGE of 4096 unitigs: how many have labels[u] == u.
//   scan     the family's scan_single_kernel over the ranges' counts: the first id of every range, and C.
//   rank     a block per range: block scan behind the range's first id -> the id of every root, stored at the root's own slot of
//            `ids` (or of a U-word array in the work buffer when the caller wants records but no ids); the root's record is
//            opened here: (root, 0, 0, 0).
//   gather   ids[u] = ids[labels[u]] for the rest, and the records: a segmented sum over the wave's lanes -- neighbouring unitigs
//            mostly share a component -- and one u64 atomicAdd per run and word.
// Integer atomics only (min, add): the results do not depend on their order, so repeated calls give identical bytes.  No LDS
// outside the two kernels that scan; no scratch.
#include "kmx_count_common.h"

namespace kmx {

namespace {

constexpr u32 COMP_RANGE = CT * 16u;   // unitigs per block of the roots / rank kernels, and per scanned partial
constexpr u64 COMP_NONE = ~0ull;       // KMX_COMPONENT_NONE

// a quarter of the lanes a device of 256 compute units holds: the kernels are gathers, and a graph beyond it strides
constexpr u64 COMP_MAX_BLOCKS = 1024;

struct CompIn {
    const u64 *link_offsets, *links;
    const uint8_t* mask;   // nullptr: every unitig is alive
    u64 n_unitigs, n_links;
};

__device__ __forceinline__ bool alive(const CompIn& in, u64 u) { return in.mask == nullptr || in.mask[u] != 0u; }

__global__ void __launch_bounds__(CT) component_init_kernel(const uint8_t* __restrict__ mask, u64 n_unitigs, u64* __restrict__ parent) {
    for (u64 u = (u64)blockIdx.x * CT + threadIdx.x; u < n_unitigs; u += (u64)gridDim.x * CT)
        parent[u] = (mask == nullptr || mask[u] != 0u) ? u : COMP_NONE;
}

// one wave that saw a difference = one more in *changes (the host compares the word with what it read a round earlier)
__device__ __forceinline__ void count_change(bool changed, unsigned long long* changes) {
    const unsigned long long any = __ballot(changed);
    if (any != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(changes, 1ull);
}

// L(t) between two link offsets: n = 0 unless the slots lie in the array, are at most four and every target names an oriented
// unitig (the list of kmx_count_clean.hip).  Flat on purpose, as there: conditions go into flags and the loads are guarded one by one.
__device__ __forceinline__ u32 list_length(const CompIn& in, u64 lo, u64 hi) {
    const bool fits = (lo <= hi) & (hi <= in.n_links) & (hi - lo <= 4u);
    const u32 n = fits ? (u32)(hi - lo) : 0u;
    bool ok = true;
#pragma unroll
    for (u32 c = 0; c < 4u; ++c)
        if (c < n) ok &= in.links[lo + c] < 2u * in.n_unitigs;
    return ok ? n : 0u;
}

__global__ void __launch_bounds__(CT) component_hook_kernel(CompIn in, u64* parent, unsigned long long* changes) {
    const u64 sweep = (u64)gridDim.x * CT, first = (u64)blockIdx.x * CT + threadIdx.x;
    // (whole waves go round together: n_unitigs rounded up to the sweep, so that the ballot below has every lane)
    for (u64 u = first; u - threadIdx.x % 64u < in.n_unitigs; u += sweep) {
        bool changed = false;
        const bool live = u < in.n_unitigs && alive(in, u);
        u64 l0 = 0, l1 = 0, l2 = 0;
        if (live) {
            l0 = in.link_offsets[2u * u];
            l1 = in.link_offsets[2u * u + 1u];
            l2 = in.link_offsets[2u * u + 2u];
        }
        const u32 na = live ? list_length(in, l0, l1) : 0u, nb = live ? list_length(in, l1, l2) : 0u;
        for (u32 c = 0; c < 8u; ++c) {
            const bool has = c < 4u ? c < na : c - 4u < nb;
            if (has) {
                const u64 v = in.links[(c < 4u ? l0 + c : l1 + (c - 4u))] >> 1;   // (< n_unitigs: list_length looked)
                if (v != u && alive(in, v)) {
                    const u64 pu = parent[u], pv = parent[v];   // (each <= its unitig: both are alive)
                    if (pu != pv) {
                        atomicMin(reinterpret_cast<unsigned long long*>(parent + max(pu, pv)), (unsigned long long)min(pu, pv));
                        changed = true;
                    }
                }
            }
        }
        count_change(changed, changes);
    }
}

__global__ void __launch_bounds__(CT) component_jump_kernel(u64 n_unitigs, u64* parent, unsigned long long* changes) {
    const u64 sweep = (u64)gridDim.x * CT, first = (u64)blockIdx.x * CT + threadIdx.x;
    for (u64 u = first; u - threadIdx.x % 64u < n_unitigs; u += sweep) {
        bool changed = false;
        if (u < n_unitigs) {
            const u64 p = parent[u];
            if (p != COMP_NONE) {          // (p <= u)
                const u64 g = parent[p];   // (g <= p: p is alive, a parent always is)
                if (g != p) {
                    parent[u] = g;         // (u's own word: no other lane of this launch writes it)
                    changed = true;
                }
            }
        }
        count_change(changed, changes);
    }
}

// how many of the 16 unitigs from u0 on are roots, and which (bit j: u0 + j)
__device__ __forceinline__ u32 roots_in(const u64* __restrict__ labels, u64 n_unitigs, u64 u0) {
    u32 bits = 0;
#pragma unroll
    for (u32 j = 0; j < 16u; ++j)
        if (u0 + j < n_unitigs && labels[u0 + j] == u0 + j) bits |= 1u << j;
    return bits;
}

__global__ void __launch_bounds__(CT) component_roots_kernel(const u64* __restrict__ labels, u64 n_unitigs, u64* __restrict__ partial) {
    __shared__ u64 sh[CT / 64];
    const u64 tot = block_sum(__popc(roots_in(labels, n_unitigs, (u64)blockIdx.x * COMP_RANGE + (u64)threadIdx.x * 16u)), sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// rank[root] = the root's id; rec (may be nullptr, else room for every id): the root's record is opened
__global__ void __launch_bounds__(CT) component_rank_kernel(const u64* __restrict__ labels, u64 n_unitigs, const u64* __restrict__ partial,
                                                            u64* __restrict__ rank, u64* __restrict__ rec) {
    __shared__ u64 sh[CT];
    const u64 u0 = (u64)blockIdx.x * COMP_RANGE + (u64)threadIdx.x * 16u;
    const u32 bits = roots_in(labels, n_unitigs, u0);
    u64 tot;
    u64 run = partial[blockIdx.x] + block_exscan(__popc(bits), sh, &tot);
#pragma unroll
    for (u32 j = 0; j < 16u; ++j) {
        if ((bits >> j & 1u) != 0u) {
            rank[u0 + j] = run;
            if (rec) {
                rec[4u * run] = u0 + j;
                rec[4u * run + 1u] = rec[4u * run + 2u] = rec[4u * run + 3u] = 0u;
            }
            ++run;
        }
    }
}

struct Sums {
    u64 n, m, s;
};

// ids (may be nullptr): the id of every unitig that is not a root -- `rank` holds the roots' (ids itself, or the work buffer's array);
// rec (may be nullptr): n_rec opened records, to which every alive unitig adds (1, m(u), S(u))
__global__ void __launch_bounds__(CT) component_gather_kernel(const u64* __restrict__ labels, u64 n_unitigs, const u64* rank, u64* ids,
                                                              const u64* __restrict__ offsets, const u64* __restrict__ sums, u64* rec, u64 n_rec) {
    const u64 sweep = (u64)gridDim.x * CT, first = (u64)blockIdx.x * CT + threadIdx.x;
    const u32 lane = threadIdx.x & 63u;
    for (u64 u = first; u - lane < n_unitigs; u += sweep) {
        const u64 lab = u < n_unitigs ? labels[u] : COMP_NONE;
        const u64 id = lab != COMP_NONE ? rank[lab] : COMP_NONE;   // (lab < n_unitigs, and a root: its slot was written by the rank kernel)
        if (ids && u < n_unitigs && lab != u) ids[u] = id;
        if (rec == nullptr) continue;   // (uniform)
        Sums w{0u, 0u, 0u};
        if (id != COMP_NONE) {
            u64 m = 1u;
            if (offsets) {
                const u64 a = offsets[u], b = offsets[u + 1u];
                m = b >= a ? b - a : 0u;
            }
            w = Sums{1u, m, sums ? sums[u] : m};
        }
        // inclusive sums over runs of equal ids: `open` = the run's head lies at or below the lanes summed so far
        const u64 before = __shfl_up(id, 1u);
        bool open = lane == 0u || before != id;
#pragma unroll
        for (u32 d = 1; d < 64u; d <<= 1) {
            const u64 xn = __shfl_up(w.n, d), xm = __shfl_up(w.m, d), xs = __shfl_up(w.s, d);
            const bool xo = __shfl_up((u32)open, d) != 0u;
            if (lane >= d && !open) {
                w.n += xn;
                w.m += xm;
                w.s += xs;
                open = xo;
            }
        }
        const u64 after = __shfl_down(id, 1u);
        if ((lane == 63u || after != id) && id < n_rec) {   // the run's last lane holds its sums (id == NONE fails the bound)
            atomicAdd(reinterpret_cast<unsigned long long*>(rec + 4u * id + 1u), (unsigned long long)w.n);
            atomicAdd(reinterpret_cast<unsigned long long*>(rec + 4u * id + 2u), (unsigned long long)w.m);
            atomicAdd(reinterpret_cast<unsigned long long*>(rec + 4u * id + 3u), (unsigned long long)w.s);
        }
    }
}

struct CompArea {
    u64* partial;                 // n_ranges + 1: the ranges' root counts, then C
    unsigned long long* changes;  // one word
    u64* rank;                    // n_unitigs words, or nullptr
    u64 n_ranges;
};
CompArea comp_area(void* area, u64 n_unitigs, bool own_rank) {
    CompArea a;
    a.n_ranges = ceil_div(n_unitigs, COMP_RANGE);
    char* p = static_cast<char*>(area);
    a.partial = reinterpret_cast<u64*>(p);
    p += align256(8u * (a.n_ranges + 1u));
    a.changes = reinterpret_cast<unsigned long long*>(p);
    p += 256u;
    a.rank = own_rank ? reinterpret_cast<u64*>(p) : nullptr;
    return a;
}

unsigned comp_blocks(u64 lanes) {
    const u64 nb = ceil_div(lanes, CT);
    return (unsigned)(nb < COMP_MAX_BLOCKS ? nb : COMP_MAX_BLOCKS);
}

}  // namespace

// the components' working set for n_unitigs unitigs: a partial per range (+ the total), the change counter and, when records are
// wanted without ids, the roots' ids
size_t count_components_bytes(u64 n_unitigs, bool own_rank) {
    return align256(8u * (ceil_div(n_unitigs, COMP_RANGE) + 1u)) + 256u + (own_rank ? align256(8u * n_unitigs) : 0u);
}

// the labels (n_unitigs >= 1) and how many components there are; *bad: the rounds ran out (no input does that).  Synchronous: one
// host round trip per round and one for the count
hipError_t launch_count_components_label(const u64* link_offsets, const u64* links, u64 n_links, const uint8_t* mask, u64 n_unitigs, u64* labels,
                                         void* area, bool own_rank, unsigned long long* h_pinned, u64* h_components, u32* h_rounds, bool* bad,
                                         hipStream_t st) {
    const CompArea a = comp_area(area, n_unitigs, own_rank);
    const CompIn in{link_offsets, links, mask, n_unitigs, n_links};
    const unsigned nb = comp_blocks(n_unitigs);
    hipError_t e = hipMemsetAsync(a.changes, 0, 8u, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(component_init_kernel, dim3(nb), dim3(CT), 0, st, mask, n_unitigs, labels);
    u64 seen = 0, now = 0;
    u32 rounds = 0;
    *bad = false;
    for (;;) {
        hipLaunchKernelGGL(component_hook_kernel, dim3(nb), dim3(CT), 0, st, in, labels, a.changes);
        hipLaunchKernelGGL(component_jump_kernel, dim3(nb), dim3(CT), 0, st, n_unitigs, labels, a.changes);
        if ((e = read_back(h_pinned, a.changes, 1u, &now, st)) != hipSuccess) return e;
        ++rounds;
        if (now == seen) break;
        seen = now;
        if ((u64)rounds > n_unitigs + 2u) {
            *bad = true;
            break;
        }
    }
    *h_rounds = rounds;
    hipLaunchKernelGGL(component_roots_kernel, dim3((unsigned)a.n_ranges), dim3(CT), 0, st, labels, n_unitigs, a.partial);
    hipLaunchKernelGGL(scan_single_kernel, dim3(1), dim3(CT), 0, st, a.partial, a.n_ranges, a.partial + a.n_ranges);
    return read_back(h_pinned, a.partial + a.n_ranges, 1u, h_components, st);
}

// after launch_count_components_label on the same arrays: the ids (may be nullptr) and the records (may be nullptr; else room for
// n_components of them); offsets and sums may be nullptr.  Asynchronous
hipError_t launch_count_components_emit(const u64* labels, u64 n_unitigs, const u64* offsets, const u64* sums, const void* area, bool own_rank, u64* ids,
                                        u64* records, u64 n_components, hipStream_t st) {
    const CompArea a = comp_area(const_cast<void*>(area), n_unitigs, own_rank);
    u64* rank = ids ? ids : a.rank;
    if (rank == nullptr) return hipSuccess;   // (neither ids nor records)
    hipLaunchKernelGGL(component_rank_kernel, dim3((unsigned)a.n_ranges), dim3(CT), 0, st, labels, n_unitigs, a.partial, rank, records);
    hipLaunchKernelGGL(component_gather_kernel, dim3(comp_blocks(n_unitigs)), dim3(CT), 0, st, labels, n_unitigs, rank, ids, offsets, sums, records,
                       records ? n_components : 0u);
    return hipGetLastError();
}

}  // namespace kmx
