// kmx_count_unitigs.hip -- the unitigs of a count table's de Bruijn graph: kmx_count_unitigs(2) (the non-branching paths as ordered
// lists of oriented nodes, with offsets, circular flags and abundance sums) and kmx_count_unitig_sequences(2) (their bases), on top of
// the three outputs of kmx_count_adjacency(2).  The definitions are in include/kmx.h; DESIGN 4.6.6 has the byte model.
//
// An oriented node is v = 2 i + o: entry i read forward (o = 0) or as its reverse complement (o = 1); mirror(v) = v ^ 1.
//
// Link.  link_out is the candidate next(v) -- present entry, a side that is no END by the rule of kmx_count_unitig_ends, a neighbour
// inside the table, neither entry a palindrome -- one lane per oriented node, into an array.  A link counts only if it is mutual,
// cand[mirror(cand[v])] == mirror(v); so next is injective whatever the inputs hold, the oriented nodes fall into disjoint simple
// chains and cycles, and neither can contain a node and its mirror (the mirror image would fix a node or an edge of it: v != v ^ 1,
// and an edge from an entry to itself is an END).  prev(v) = mirror(next(mirror(v))): one gather.
//
// Rank.  Pointer jumping backwards, one 16-byte record per oriented node, two buffers (a round reads one and writes the other):
//   done   {head of the chain, distance to it}: final; a round copies it without a gather;
//   open   {prev^(2^r)(v), m = the smallest node among v, prev(v), .. prev^(2^r - 1)(v), and how many steps back m is}
// after r rounds.  An open node whose pointer is done becomes done (its distance is 2^r + the pointer's); otherwise it takes the
// pointer's pointer and the smaller m.  Chain nodes finish in distance order (all within 2^r after round r); the nodes that never
// finish lie on cycles, and there the same doubling spreads the cycle's smallest node and every node's distance from it -- the
// cycle written from its minimum -- so cycles cost no second ranking.  Every round adds {newly done, m changed} to a record of its
// own that the host reads back; it stops when no open node is left, or when a round finishes none and changes none (then every
// window's minimum equals that of the window 2^r further back, whose union along the steps is the whole cycle).  At most
// ceil(log2(longest chain or cycle)) + 2 rounds, 43 for 2^41 nodes.
//
// Compact.  Per entry: is it the head of a canonical unitig (the chain whose head entry is the smaller of its own and its mirror's,
// i.e. head < tail by entry; the cycle whose minimum is an even node), and how long is that -- a block sum per 256 entries, one scan
// of the partials, then ids and offsets; a lane per oriented node scatters itself to offset[head] + distance and adds its count.
//
// Vector loads and stores and u64 device atomics only; no LDS beyond the block scans; no scratch.  Every index read from an input is
// checked against n before it is used.
#include "kmx_count_common.h"

namespace kmx {

namespace {

constexpr u64 NO_NODE = ~0ull;
constexpr u32 UT_ROUNDS = 43;              // rounds are numbered 0 .. 42: a distance or a step count stays below 2^42
constexpr u32 UT_REC_UNDONE = 0;           // the words of the record block at the head of the work area
constexpr u32 UT_REC_ROUND = 2;            // + 2 r: {newly done, minimum changed} of round r
constexpr u32 UT_REC_TOTALS = 100;         // {unitigs, nodes}
constexpr size_t UT_REC_BYTES = 1024;

// ---------------------------------------------------------------- the rank record
struct alignas(16) Rank {
    u64 a, b;
};
constexpr u64 R_DONE = 1ull << 63;
constexpr u32 R_ID = 41, R_OFF = 42, R_MN_LOW = 64u - R_OFF;   // a node id has 41 bits; 22 bits of m ride above the step count
constexpr u64 R_ID_MASK = (1ull << R_ID) - 1ull, R_OFF_MASK = (1ull << R_OFF) - 1ull;

__device__ __forceinline__ Rank rank_done(u64 head, u64 dist) { return Rank{head | R_DONE, dist}; }
__device__ __forceinline__ Rank rank_open(u64 ptr, u64 mn, u64 off) { return Rank{ptr | ((mn >> R_MN_LOW) << R_ID), off | (mn << R_OFF)}; }
__device__ __forceinline__ bool is_done(const Rank& r) { return (r.a >> 63) != 0u; }
__device__ __forceinline__ u64 ptr_of(const Rank& r) { return r.a & R_ID_MASK; }
__device__ __forceinline__ u64 open_mn(const Rank& r) { return ((r.a >> R_ID) << R_MN_LOW) | (r.b >> R_OFF); }   // (open: bit 63 of a is 0)
__device__ __forceinline__ u64 open_off(const Rank& r) { return r.b & R_OFF_MASK; }
// the head (a cycle: its smallest node) and the distance from it
__device__ __forceinline__ u64 head_of(const Rank& r) { return is_done(r) ? ptr_of(r) : open_mn(r); }
__device__ __forceinline__ u64 dist_of(const Rank& r) { return is_done(r) ? r.b : open_off(r); }

// ---------------------------------------------------------------- links
__device__ __forceinline__ bool entry_present(const u64* __restrict__ counts, u64 min_count, u64 i) { return counts == nullptr || counts[i] >= min_count; }

template <u32 W>
__device__ __forceinline__ bool palindrome(const u64* __restrict__ keys, u64 i, u32 k) {
    const Key<W> x = Key<W>::load(keys, i);
    return x.revcomp(k).equal(x);
}

// The candidate next(v), NO_NODE if there is none: everything but mutuality.  EVEN: k is even, palindromes exist and keys is read.
template <u32 W, bool EVEN>
__device__ __forceinline__ u64 link_out(const u64* __restrict__ keys, const u64* __restrict__ counts, u64 min_count, const uint8_t* __restrict__ edges,
                                        const uint8_t* __restrict__ flips, const u64* __restrict__ nbr, u64 n, u32 k, u64 v) {
    const u64 i = v >> 1;
    const u32 o = (u32)v & 1u;
    if (!entry_present(counts, min_count, i)) return NO_NODE;
    const u32 nib = ((u32)edges[i] >> (4u * o)) & 15u;
    if (__popc(nib) != 1) return NO_NODE;
    const u32 e = 4u * o + (u32)__ffs((int)nib) - 1u;
    const u64 j = nbr[8u * i + e];
    if (j >= n || j == i) return NO_NODE;
    const u32 f = ((u32)flips[i] >> e) & 1u;
    // (kmx_count_unitig_ends: a successor edge enters its neighbour at the predecessor side, a flipped one at the other)
    const u32 other = edges[j];
    if (__popc((o ^ f) == 0u ? other >> 4 : other & 15u) != 1) return NO_NODE;
    if (EVEN && (palindrome<W>(keys, i, k) || palindrome<W>(keys, j, k))) return NO_NODE;
    return 2u * j + (u64)(o ^ f);
}

// next(v) of a node that is known to have one (its link was found mutual): no checks but the bound
__device__ __forceinline__ u64 link_follow(const uint8_t* __restrict__ edges, const uint8_t* __restrict__ flips, const u64* __restrict__ nbr, u64 n, u64 v) {
    const u64 i = v >> 1;
    const u32 o = (u32)v & 1u;
    const u32 nib = ((u32)edges[i] >> (4u * o)) & 15u;
    if (nib == 0u) return NO_NODE;
    const u32 e = 4u * o + (u32)__ffs((int)nib) - 1u;
    const u64 j = nbr[8u * i + e];
    if (j >= n) return NO_NODE;
    return 2u * j + (u64)(o ^ (((u32)flips[i] >> e) & 1u));
}

template <u32 W, bool EVEN>
__global__ void __launch_bounds__(CT) link_kernel(const u64* __restrict__ keys, const u64* __restrict__ counts, u64 min_count, const uint8_t* __restrict__ edges,
                                                  const uint8_t* __restrict__ flips, const u64* __restrict__ nbr, u64 n, u32 k, u64* __restrict__ cand) {
    for (u64 v = (u64)blockIdx.x * CT + threadIdx.x; v < 2u * n; v += (u64)gridDim.x * CT)
        cand[v] = link_out<W, EVEN>(keys, counts, min_count, edges, flips, nbr, n, k, v);
}

// prev(v) from the candidates, and the first rank record: a node without one is the head of its chain
__global__ void __launch_bounds__(CT) rank_init_kernel(const u64* __restrict__ cand, u64 n_nodes, Rank* __restrict__ out, unsigned long long* __restrict__ rec) {
    __shared__ u64 sh[CT / 64u];
    u64 undone = 0;
    for (u64 v = (u64)blockIdx.x * CT + threadIdx.x; v < n_nodes; v += (u64)gridDim.x * CT) {
        const u64 w = cand[v ^ 1u];   // next(mirror(v)), if it is mutual: next(mirror(w)) == v
        const bool linked = w < n_nodes && cand[w ^ 1u] == v;
        out[v] = linked ? rank_open(w ^ 1u, v, 0u) : rank_done(v, 0u);
        if (linked) ++undone;
    }
    undone = block_sum(undone, sh);
    if (threadIdx.x == 0 && undone != 0u) atomicAdd(&rec[UT_REC_UNDONE], (unsigned long long)undone);
}

// round r: d = 2^r
__global__ void __launch_bounds__(CT) rank_round_kernel(const Rank* __restrict__ cur, Rank* __restrict__ nxt, u64 n_nodes, u64 d, unsigned long long* __restrict__ rec) {
    __shared__ u64 sh[CT / 64u];
    u64 fin = 0, chg = 0;
    for (u64 v = (u64)blockIdx.x * CT + threadIdx.x; v < n_nodes; v += (u64)gridDim.x * CT) {
        Rank s = cur[v];
        if (!is_done(s)) {
            const Rank q = cur[ptr_of(s)];
            if (is_done(q)) {
                s = rank_done(ptr_of(q), d + q.b);
                ++fin;
            } else {
                u64 mn = open_mn(s), off = open_off(s);
                const u64 qm = open_mn(q);
                if (qm < mn) {
                    mn = qm;
                    off = d + open_off(q);
                    ++chg;
                }
                s = rank_open(ptr_of(q), mn, off);
            }
        }
        nxt[v] = s;
    }
    fin = block_sum(fin, sh);
    if (threadIdx.x == 0 && fin != 0u) atomicAdd(&rec[0], (unsigned long long)fin);
    chg = block_sum(chg, sh);
    if (threadIdx.x == 0 && chg != 0u) atomicAdd(&rec[1], (unsigned long long)chg);
}

// ---------------------------------------------------------------- compaction
// info[i] after heads_mark_kernel: {a = 1 (entry i heads a canonical unitig) | o << 1 | circular << 2, b = its length}; after
// heads_place_kernel: {a = the unitig's id, NO_NODE if it heads none, b = offset << 1 | o}.
__global__ void __launch_bounds__(CT) heads_mark_kernel(const Rank* __restrict__ rank, const u64* __restrict__ counts, u64 min_count,
                                                        const uint8_t* __restrict__ edges, const uint8_t* __restrict__ flips, const u64* __restrict__ nbr, u64 n,
                                                        Rank* __restrict__ info, u64* __restrict__ part_heads, u64* __restrict__ part_nodes) {
    __shared__ u64 sh[CT / 64u];
    const u64 n_tiles = ceil_div(n, CT);
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const u64 i = tile * CT + threadIdx.x;
        u64 flag = 0, len = 0;
        if (i < n && entry_present(counts, min_count, i)) {
#pragma unroll
            for (u32 o = 0; o < 2u; ++o) {
                const u64 h = 2u * i + o;
                const Rank s = rank[h];
                if (flag != 0u) continue;
                if (is_done(s)) {
                    if (ptr_of(s) != h) continue;             // inside a chain
                    const Rank m = rank[h ^ 1u];               // the tail of the mirror chain: its head is mirror(tail of this one)
                    const u64 ti = head_of(m) >> 1;
                    if (i < ti || (i == ti && o == 0u)) {
                        flag = 1u | (o << 1);
                        len = dist_of(m) + 1u;
                    }
                } else if (o == 0u && open_mn(s) == h) {       // the smallest node of a cycle, and even: the canonical one starts here
                    const u64 w = link_follow(edges, flips, nbr, n, h ^ 1u);   // prev(h) = mirror(next(mirror(h))): the last node
                    if (w < 2u * n) {
                        flag = 1u | 4u;
                        len = dist_of(rank[w ^ 1u]) + 1u;
                    }
                }
            }
        }
        if (i < n) info[i] = Rank{flag, len};
        const u64 f = block_sum(flag & 1u, sh);
        if (threadIdx.x == 0) part_heads[tile] = f;
        const u64 l = block_sum(len, sh);
        if (threadIdx.x == 0) part_nodes[tile] = l;
    }
}

// part_*: scanned (exclusive); totals = {unitigs, nodes}
__global__ void __launch_bounds__(CT) heads_place_kernel(Rank* __restrict__ info, u64 n, const u64* __restrict__ part_heads, const u64* __restrict__ part_nodes,
                                                         const unsigned long long* __restrict__ totals, u64* __restrict__ offsets, uint8_t* __restrict__ circular,
                                                         unsigned long long* __restrict__ sums) {
    __shared__ u64 sh[CT];
    const u64 n_tiles = ceil_div(n, CT);
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const u64 i = tile * CT + threadIdx.x;
        const Rank in = i < n ? info[i] : Rank{0u, 0u};
        u64 tot;
        const u64 id = part_heads[tile] + block_exscan(in.a & 1u, sh, &tot);
        const u64 at = part_nodes[tile] + block_exscan(in.b, sh, &tot);
        if (i < n) {
            const bool head = (in.a & 1u) != 0u;
            info[i] = Rank{head ? id : NO_NODE, (at << 1) | ((in.a >> 1) & 1u)};
            if (head) {
                offsets[id] = at;
                if (circular) circular[id] = (uint8_t)((in.a >> 2) & 1u);
                if (sums) sums[id] = 0u;
            }
            if (i == n - 1u) offsets[totals[0]] = totals[1];
        }
    }
}

__global__ void __launch_bounds__(CT) scatter_kernel(const Rank* __restrict__ rank, const Rank* __restrict__ info, const u64* __restrict__ counts, u64 n,
                                                     u64* __restrict__ nodes, unsigned long long* __restrict__ sums) {
    for (u64 v = (u64)blockIdx.x * CT + threadIdx.x; v < 2u * n; v += (u64)gridDim.x * CT) {
        const Rank s = rank[v];
        const u64 h = head_of(s);
        const Rank at = info[h >> 1];
        if (at.a == NO_NODE || (at.b & 1u) != (h & 1u)) continue;   // the mirror of a canonical unitig, or an entry that is not present
        const u64 pos = (at.b >> 1) + dist_of(s);
        if (pos >= n) continue;
        nodes[pos] = v;
        if (sums) atomicAdd(&sums[at.a], (unsigned long long)(counts ? counts[v >> 1] : 1u));
    }
}

// ---------------------------------------------------------------- the sequences
// A lane per output node t: its unitig u by a search of the offsets, then the top base of its word behind the k bases of the
// unitig's first word (which that node's lane writes): unitig u starts at byte offsets[u] + u (k - 1).
template <u32 W>
__global__ void __launch_bounds__(CT) spell_kernel(const u64* __restrict__ keys, u64 n, u32 k, const u64* __restrict__ nodes, const u64* __restrict__ offsets,
                                                   u64 n_unitigs, uint8_t* __restrict__ seq) {
    using K = Key<W>;
    constexpr u32 ACGT = 0x54474341u;
    const u64 total = offsets[n_unitigs];
    for (u64 t = (u64)blockIdx.x * CT + threadIdx.x; t < total && t < n; t += (u64)gridDim.x * CT) {
        const u64 v = nodes[t];
        if ((v >> 1) >= n) continue;
        u64 lo = 0, hi = n_unitigs;   // offsets[lo] <= t < offsets[hi]
        while (hi - lo > 1u) {
            const u64 mid = lo + ((hi - lo) >> 1);
            if (offsets[mid] <= t) lo = mid;
            else hi = mid;
        }
        const u64 first = offsets[lo];
        uint8_t* out = seq + first + lo * (u64)(k - 1u);
        const K x = K::load(keys, v >> 1);
        if (t == first) {
            const K w = (v & 1u) ? x.revcomp(k) : x;
            for (u32 b = 0; b < k; ++b) out[b] = (uint8_t)(ACGT >> (8u * (w.bits(2u * b) & 3u)));
        } else {
            const u32 c = (v & 1u) ? 3u - (x.bits(0u) & 3u) : x.top_base(k);   // (the top base of rc(x) is the complement of x's lowest)
            out[(u64)(k - 1u) + (t - first)] = (uint8_t)(ACGT >> (8u * c));
        }
    }
}

// a lane per item; above 2^30 blocks the lanes loop
unsigned lane_grid(u64 items) {
    const u64 nb = ceil_div(items, CT);
    return (unsigned)(nb < (1ull << 30) ? nb : (1ull << 30));
}

}  // namespace

// ---------------------------------------------------------------- host side
// The work area: [records][rank buffer A: 16 bytes per oriented node][rank buffer B: the same; first the link candidates, at the end
// the heads' ids and offsets][partial sums: 2 u64 per 256 entries].  64 bytes per entry and a little.
size_t count_unitigs_bytes(u64 n) { return UT_REC_BYTES + 2u * align256(32u * (size_t)n) + 2u * align256(8u * (size_t)ceil_div(n, CT)); }

// *bad: the rounds ran out (a state this code cannot reach; nothing is written to the outputs then)
hipError_t launch_count_unitigs(u32 words, const u64* keys, const u64* counts, u64 n, u32 k, u64 min_count, const uint8_t* edges, const uint8_t* flips,
                                const u64* nbr, u64* nodes, u64* offsets, uint8_t* circular, u64* sums, void* area, unsigned long long* h_pinned,
                                u64* n_unitigs, u64* n_nodes, u32* rounds, bool* bad, hipStream_t st) {
    char* base = static_cast<char*>(area);
    unsigned long long* rec = reinterpret_cast<unsigned long long*>(base);
    Rank* cur = reinterpret_cast<Rank*>(base + UT_REC_BYTES);
    Rank* nxt = reinterpret_cast<Rank*>(base + UT_REC_BYTES + align256(32u * (size_t)n));
    u64* part_heads = reinterpret_cast<u64*>(base + UT_REC_BYTES + 2u * align256(32u * (size_t)n));
    u64* part_nodes = part_heads + align256(8u * (size_t)ceil_div(n, CT)) / 8u;
    const u64 n_nodes2 = 2u * n, n_tiles = ceil_div(n, CT);
    const dim3 block(CT), per_node(lane_grid(n_nodes2)), per_tile((unsigned)(n_tiles < (1ull << 30) ? n_tiles : (1ull << 30)));
    *bad = false;
    *rounds = 0;
    hipError_t e = hipMemsetAsync(rec, 0, UT_REC_BYTES, st);
    if (e != hipSuccess) return e;
    u64* cand = reinterpret_cast<u64*>(nxt);
    const bool even = (k & 1u) == 0u;
    with_width(words, [&](auto w) {
        constexpr u32 W = decltype(w)::value;
        if (even) hipLaunchKernelGGL((link_kernel<W, true>), per_node, block, 0, st, keys, counts, min_count, edges, flips, nbr, n, k, cand);
        else hipLaunchKernelGGL((link_kernel<W, false>), per_node, block, 0, st, keys, counts, min_count, edges, flips, nbr, n, k, cand);
    });
    hipLaunchKernelGGL(rank_init_kernel, per_node, block, 0, st, cand, n_nodes2, cur, rec);
    u64 open = 0;
    if ((e = read_back(h_pinned, rec + UT_REC_UNDONE, 1u, &open, st)) != hipSuccess) return e;
    u32 r = 0;
    while (open != 0u) {
        if (r >= UT_ROUNDS) {
            *bad = true;
            return hipSuccess;
        }
        unsigned long long* rr = rec + UT_REC_ROUND + 2u * r;
        hipLaunchKernelGGL(rank_round_kernel, per_node, block, 0, st, cur, nxt, n_nodes2, 1ull << r, rr);
        u64 got[2];
        if ((e = read_back(h_pinned, rr, 2u, got, st)) != hipSuccess) return e;
        Rank* t = cur;
        cur = nxt;
        nxt = t;
        ++r;
        open -= got[0] < open ? got[0] : open;
        if (got[0] == 0u && got[1] == 0u) break;   // what is open now lies on cycles, and every cycle knows its smallest node
    }
    *rounds = r;
    Rank* info = nxt;
    hipLaunchKernelGGL(heads_mark_kernel, per_tile, block, 0, st, cur, counts, min_count, edges, flips, nbr, n, info, part_heads, part_nodes);
    hipLaunchKernelGGL(scan_single_kernel, dim3(1), block, 0, st, part_heads, n_tiles, reinterpret_cast<u64*>(rec + UT_REC_TOTALS));
    hipLaunchKernelGGL(scan_single_kernel, dim3(1), block, 0, st, part_nodes, n_tiles, reinterpret_cast<u64*>(rec + UT_REC_TOTALS + 1u));
    hipLaunchKernelGGL(heads_place_kernel, per_tile, block, 0, st, info, n, part_heads, part_nodes, rec + UT_REC_TOTALS, offsets, circular,
                       reinterpret_cast<unsigned long long*>(sums));
    hipLaunchKernelGGL(scatter_kernel, per_node, block, 0, st, cur, info, counts, n, nodes, reinterpret_cast<unsigned long long*>(sums));
    u64 tot[2];
    if ((e = read_back(h_pinned, rec + UT_REC_TOTALS, 2u, tot, st)) != hipSuccess) return e;
    *n_unitigs = tot[0];
    *n_nodes = tot[1];
    return hipSuccess;
}

hipError_t launch_count_unitig_sequences(u32 words, const u64* keys, u64 n, u32 k, const u64* nodes, const u64* offsets, u64 n_unitigs, uint8_t* seq,
                                         hipStream_t st) {
    with_width(words, [&](auto w) {
        constexpr u32 W = decltype(w)::value;
        hipLaunchKernelGGL(spell_kernel<W>, dim3(lane_grid(n)), dim3(CT), 0, st, keys, n, k, nodes, offsets, n_unitigs, seq);
    });
    return hipGetLastError();
}

}  // namespace kmx
