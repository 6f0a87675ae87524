// kmx_count_setop.hip -- what relates TWO count tables (keys ascending and distinct, one u64 count per key): kmx_count_setop(2)
// (intersection, union, difference, symmetric difference, difference of counts) and kmx_count_compare(2) (the nine sums behind
// Jaccard, containment and weighted Jaccard).  One sequential pass over each table per kernel; nothing of the size of the inputs
// is kept between kernels -- 24 bytes of work buffer per TILE of SETOP_TILE merged entries.
//
// Partition.  The merged sequence of n_a + n_b entries (ties: `a` first, as merge_kernel) is cut at the diagonals m * SETOP_TILE;
//   one thread per cut finds its merge-path split (i_a, i_b) by binary search.  With that tie rule an equal pair can straddle a
//   cut (a[i_a - 1] == b[i_b]): the cut then moves one step along `b`, so the pair belongs WHOLE to the tile that holds a's entry
//   and the next tile starts behind b's.  A tile so holds at most SETOP_TILE + 1 entries and no tile ever looks outside its ranges.
// Tile.  A block loads its two key ranges into LDS with coalesced loads (8 bytes per lane for one-word keys: a tile starts at any
//   entry, so 16-byte loads of one-word keys would need a peeled head; 16 bytes per lane for two-word keys), each thread finds the
//   split of its own diagonal in LDS -- the same search and the same step along `b` -- and walks at most SETOP_IPT + 1 entries.
//   Counts go to LDS as well only where the DECISION needs them (COUNTER_SUBTRACT, compare).
// Count pass: the walk counts what the operation emits; per-tile totals (block_sum of kmx_count_common.h), scan_single_kernel,
//   the host reads n_out.
// Write pass: the walk again, leaving one 32-bit descriptor (index in a's range, index in b's range; 0xFFFF = none) per emitted
//   entry at its scanned place in LDS; then the block writes the tile's output in order -- keys from LDS, counts gathered from the
//   two count arrays at ascending indices, the rule applied -- so what leaves is whole lines of keys and counts.
// Compare: the count pass with counts, six sums per thread folded per block (wave_sum_shfl of kmx_count_common.h, then LDS) and
//   added to the record with six device atomics (integer adds: any order gives the same record).  The host derives the other
//   three (n_only_* from n_a, n_b; sum_max from sum_a + sum_b - sum_min).
// Tables that are not sorted give wrong answers, never an access outside the arrays: every range is clamped to what LDS holds
// before it is used, a walk is at most SETOP_IPT + 1 steps whatever the keys say, and both passes make the same decisions, so the
// write pass stays inside the n_out the count pass reported.  No scratch, no pass waits on another block.
#include "kmx_count_common.h"

namespace kmx {

namespace {

constexpr u32 SETOP_IPT = 8;                  // merged entries per thread (one more when a pair is pulled over a cut)
constexpr u32 SETOP_TILE = CT * SETOP_IPT;    // merged entries per tile: 2048 (kmers_amd/_lib.py SETOP_TILE, for the boundary tests)
constexpr u32 SETOP_SLOTS = SETOP_TILE + 1;   // entries a tile can hold
constexpr u32 SETOP_WALK = SETOP_IPT + 1;     // steps of a thread's walk
constexpr u32 SETOP_NONE = 0xFFFFu;           // "no entry of this table" in a descriptor
static_assert(SETOP_SLOTS < SETOP_NONE, "a tile's indices fit 16 bits");

// ---------------------------------------------------------------- the partition
// split[2 m], split[2 m + 1] = how many entries of a / of b lie before cut m, m = 0 .. n_tiles
template <u32 W>
__global__ void __launch_bounds__(CT) setop_partition_kernel(const u64* __restrict__ ka, u64 na, const u64* __restrict__ kb, u64 nb, u64 n_tiles,
                                                             u64* __restrict__ split) {
    using K = Key<W>;
    const u64 m = (u64)blockIdx.x * CT + threadIdx.x;
    if (m > n_tiles) return;
    const u64 n = na + nb;
    u64 d = m * SETOP_TILE;
    if (d > n) d = n;
    u64 lo = d > nb ? d - nb : 0u, hi = d < na ? d : na;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;   // (lo <= mid < hi: d - nb <= mid <= d - 1, so 0 <= d - 1 - mid < nb)
        if (!K::load(kb, d - 1u - mid).less(K::load(ka, mid))) lo = mid + 1u;   // a[mid] <= b[d - 1 - mid]
        else hi = mid;
    }
    u64 i = lo, j = d - lo;
    if (i > 0u && j < nb && K::load(ka, i - 1u).equal(K::load(kb, j))) ++j;   // the pair stays with a's entry
    split[2u * m] = i;
    split[2u * m + 1u] = j;
}

// ---------------------------------------------------------------- a tile in LDS
struct TileRange {
    u64 a0, b0;   // first entry of the tile in a / in b
    u32 na, nb;   // entries of a / of b in the tile: na + nb <= SETOP_SLOTS
};

// (sorted tables: cuts ascend and a tile holds at most SETOP_SLOTS entries; anything else is clamped to that, inside the arrays:
// a0 + na <= the next cut's i_a <= n_a)
__device__ __forceinline__ TileRange tile_range(const u64* __restrict__ split, u64 t) {
    const u64 a0 = split[2u * t], b0 = split[2u * t + 1u], a1 = split[2u * t + 2u], b1 = split[2u * t + 3u];
    u64 na = a1 > a0 ? a1 - a0 : 0u;
    if (na > SETOP_SLOTS) na = SETOP_SLOTS;
    u64 nb = b1 > b0 ? b1 - b0 : 0u;
    if (nb > SETOP_SLOTS - na) nb = SETOP_SLOTS - na;
    return TileRange{a0, b0, (u32)na, (u32)nb};
}

// keys[0 .. na) = a's range, keys[na .. na + nb) = b's; cnt likewise where the walk decides by counts (a NULL count array reads as 0)
template <u32 W, bool CNT>
__device__ __forceinline__ void tile_load(const TileRange& r, const u64* __restrict__ ka, const u64* __restrict__ ca, const u64* __restrict__ kb,
                                          const u64* __restrict__ cb, Key<W>* keys, u64* cnt) {
    for (u32 s = threadIdx.x; s < r.na; s += CT) {
        keys[s] = Key<W>::load(ka, r.a0 + s);
        if (CNT) cnt[s] = ca != nullptr ? ca[r.a0 + s] : 0u;
    }
    for (u32 s = threadIdx.x; s < r.nb; s += CT) {
        keys[r.na + s] = Key<W>::load(kb, r.b0 + s);
        if (CNT) cnt[r.na + s] = cb != nullptr ? cb[r.b0 + s] : 0u;
    }
    __syncthreads();
}

// Every thread's split at its diagonal threadIdx.x * SETOP_IPT of the tile (the partition's search and step, in LDS), left in
// splits[0 .. CT] as i | j << 16 with splits[CT] = the tile's end; returns with the splits visible to the block.
template <u32 W>
__device__ __forceinline__ void thread_splits(const Key<W>* A, u32 na, const Key<W>* B, u32 nb, u32* splits) {
    u32 d = threadIdx.x * SETOP_IPT;
    if (d > na + nb) d = na + nb;
    u32 lo = d > nb ? d - nb : 0u, hi = d < na ? d : na;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (!B[d - 1u - mid].less(A[mid])) lo = mid + 1u;
        else hi = mid;
    }
    u32 i = lo, j = d - lo;
    if (i > 0u && j < nb && A[i - 1u].equal(B[j])) ++j;
    splits[threadIdx.x] = i | (j << 16);
    if (threadIdx.x == 0) splits[CT] = na | (nb << 16);
    __syncthreads();
}

// One step of a thread's walk over [i, ie) of A and [j, je) of B: the next distinct key, ascending, as (*ai, *bj) = its index in A /
// in B or SETOP_NONE; false when both ranges are used up.  A walk is at most SETOP_WALK steps (sorted tables need no more).
template <u32 W>
__device__ __forceinline__ bool walk_step(const Key<W>* A, const Key<W>* B, u32& i, u32 ie, u32& j, u32 je, u32* ai, u32* bj) {
    const bool ha = i < ie, hb = j < je;
    if (!ha && !hb) return false;
    bool ta = ha, tb = hb;
    if (ha && hb) {
        const Key<W> x = A[i], y = B[j];
        ta = !y.less(x);   // a's key <= b's
        tb = !x.less(y);
    }
    *ai = ta ? i : SETOP_NONE;
    *bj = tb ? j : SETOP_NONE;
    i += ta ? 1u : 0u;
    j += tb ? 1u : 0u;
    return true;
}

// does the operation emit this key?  (cnt: the tile's counts in LDS, COUNTER_SUBTRACT only)
template <u32 OP>
__device__ __forceinline__ bool emits(u32 ai, u32 bj, const u64* cnt, u32 na) {
    const bool a = ai != SETOP_NONE, b = bj != SETOP_NONE;
    if (OP == KMX_SETOP_INTERSECT) return a && b;
    if (OP == KMX_SETOP_UNION) return true;
    if (OP == KMX_SETOP_SUBTRACT) return a && !b;
    if (OP == KMX_SETOP_SYMDIFF) return a != b;
    return a && (!b || cnt[ai] > cnt[na + bj]);   // KMX_SETOP_COUNTER_SUBTRACT
}

// ---------------------------------------------------------------- the count pass
template <u32 W, u32 OP>
__global__ void __launch_bounds__(CT) setop_count_kernel(const u64* __restrict__ ka, const u64* __restrict__ ca, const u64* __restrict__ kb,
                                                         const u64* __restrict__ cb, const u64* __restrict__ split, u64* __restrict__ partial) {
    constexpr bool CNT = OP == KMX_SETOP_COUNTER_SUBTRACT;
    __shared__ Key<W> keys[SETOP_SLOTS];
    __shared__ u64 cnt[CNT ? SETOP_SLOTS : 1];
    __shared__ u32 splits[CT + 1];
    __shared__ u64 sh[CT / 64];
    const TileRange r = tile_range(split, blockIdx.x);
    tile_load<W, CNT>(r, ka, ca, kb, cb, keys, cnt);
    const Key<W>*A = keys, *B = keys + r.na;
    thread_splits<W>(A, r.na, B, r.nb, splits);
    const u32 s0 = splits[threadIdx.x], s1 = splits[threadIdx.x + 1];
    const u32 ie = s1 & 0xFFFFu, je = s1 >> 16;
    u32 i = s0 & 0xFFFFu, j = s0 >> 16, ai, bj, c = 0;
    for (u32 s = 0; s < SETOP_WALK && walk_step<W>(A, B, i, ie, j, je, &ai, &bj); ++s) c += emits<OP>(ai, bj, cnt, r.na) ? 1u : 0u;
    const u64 tot = block_sum(c, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// ---------------------------------------------------------------- the write pass
__device__ __forceinline__ u64 ruled(u32 rule, const u64* __restrict__ ca, u64 ia, const u64* __restrict__ cb, u64 ib) {
    switch (rule) {   // (wave-uniform; a count array the rule does not name is not read: it may be NULL)
        case KMX_RULE_SUM: return ca[ia] + cb[ib];
        case KMX_RULE_MIN: {
            const u64 x = ca[ia], y = cb[ib];
            return x < y ? x : y;
        }
        case KMX_RULE_MAX: {
            const u64 x = ca[ia], y = cb[ib];
            return x > y ? x : y;
        }
        case KMX_RULE_LEFT: return ca[ia];
        default: return cb[ib];   // KMX_RULE_RIGHT
    }
}

template <u32 W, u32 OP>
__global__ void __launch_bounds__(CT) setop_write_kernel(const u64* __restrict__ ka, const u64* __restrict__ ca, const u64* __restrict__ kb,
                                                         const u64* __restrict__ cb, const u64* __restrict__ split, const u64* __restrict__ partial,
                                                         u32 rule, u64* __restrict__ out_k, u64* __restrict__ out_c) {
    constexpr bool CNT = OP == KMX_SETOP_COUNTER_SUBTRACT;
    __shared__ Key<W> keys[SETOP_SLOTS];
    __shared__ u64 cnt[CNT ? SETOP_SLOTS : 1];
    __shared__ u32 splits[CT + 1];
    __shared__ u32 desc[CT * SETOP_WALK];   // (what the walks of a block can emit at most, whatever the keys)
    __shared__ u64 sh[CT];
    const TileRange r = tile_range(split, blockIdx.x);
    tile_load<W, CNT>(r, ka, ca, kb, cb, keys, cnt);
    const Key<W>*A = keys, *B = keys + r.na;
    thread_splits<W>(A, r.na, B, r.nb, splits);
    const u32 s0 = splits[threadIdx.x], s1 = splits[threadIdx.x + 1];
    const u32 ie = s1 & 0xFFFFu, je = s1 >> 16;
    u32 i = s0 & 0xFFFFu, j = s0 >> 16, ai, bj, c = 0;
    for (u32 s = 0; s < SETOP_WALK && walk_step<W>(A, B, i, ie, j, je, &ai, &bj); ++s) c += emits<OP>(ai, bj, cnt, r.na) ? 1u : 0u;
    u64 tot;
    u32 o = (u32)block_exscan(c, sh, &tot);
    i = s0 & 0xFFFFu, j = s0 >> 16;
    for (u32 s = 0; s < SETOP_WALK && walk_step<W>(A, B, i, ie, j, je, &ai, &bj); ++s)
        if (emits<OP>(ai, bj, cnt, r.na)) desc[o++] = ai | (bj << 16);
    __syncthreads();
    const u64 base = partial[blockIdx.x];
    for (u32 s = threadIdx.x; s < (u32)tot; s += CT) {
        const u32 d = desc[s], ai = d & 0xFFFFu, bj = d >> 16;
        const bool a = ai != SETOP_NONE, b = bj != SETOP_NONE;
        u64 v;
        if (a && b) v = CNT ? cnt[ai] - cnt[r.na + bj] : ruled(rule, ca, r.a0 + ai, cb, r.b0 + bj);
        else if (a) v = ca[r.a0 + ai];
        else v = cb[r.b0 + bj];
        Key<W>::store(out_k, base + s, a ? A[ai] : B[bj]);
        out_c[base + s] = v;
    }
}

// ---------------------------------------------------------------- compare
constexpr u32 CMP_WORDS = 6;   // n_both, sum_a, sum_b, sum_a_both, sum_b_both, sum_min
static_assert(8u * CMP_WORDS <= KMX_PIN_BYTES - 8u, "the record is read back into the context's pinned words");

template <u32 W>
__global__ void __launch_bounds__(CT) setop_compare_kernel(const u64* __restrict__ ka, const u64* __restrict__ ca, const u64* __restrict__ kb,
                                                           const u64* __restrict__ cb, const u64* __restrict__ split,
                                                           unsigned long long* __restrict__ rec) {
    __shared__ Key<W> keys[SETOP_SLOTS];
    __shared__ u64 cnt[SETOP_SLOTS];
    __shared__ u32 splits[CT + 1];
    __shared__ u64 red[CT / 64][CMP_WORDS];
    const TileRange r = tile_range(split, blockIdx.x);
    tile_load<W, true>(r, ka, ca, kb, cb, keys, cnt);
    const Key<W>*A = keys, *B = keys + r.na;
    thread_splits<W>(A, r.na, B, r.nb, splits);
    const u32 s0 = splits[threadIdx.x], s1 = splits[threadIdx.x + 1];
    u64 n_both = 0, sum_a = 0, sum_b = 0, sum_ab = 0, sum_bb = 0, sum_min = 0;
    const u64* cnt_b = cnt + r.na;
    const u32 ie = s1 & 0xFFFFu, je = s1 >> 16;
    u32 i = s0 & 0xFFFFu, j = s0 >> 16, ai, bj;
    for (u32 s = 0; s < SETOP_WALK && walk_step<W>(A, B, i, ie, j, je, &ai, &bj); ++s) {
        const bool a = ai != SETOP_NONE, b = bj != SETOP_NONE;
        const u64 x = a ? cnt[ai] : 0u, y = b ? cnt_b[bj] : 0u;
        sum_a += x;
        sum_b += y;
        if (a && b) {
            n_both += 1u;
            sum_ab += x;
            sum_bb += y;
            sum_min += x < y ? x : y;
        }
    }
    n_both = wave_sum_shfl(n_both), sum_a = wave_sum_shfl(sum_a), sum_b = wave_sum_shfl(sum_b);
    sum_ab = wave_sum_shfl(sum_ab), sum_bb = wave_sum_shfl(sum_bb), sum_min = wave_sum_shfl(sum_min);
    if ((threadIdx.x & 63u) == 0u) {
        u64* w = red[threadIdx.x >> 6];
        w[0] = n_both, w[1] = sum_a, w[2] = sum_b, w[3] = sum_ab, w[4] = sum_bb, w[5] = sum_min;
    }
    __syncthreads();
    if (threadIdx.x < CMP_WORDS) {
        u64 t = 0;
        for (u32 w = 0; w < CT / 64u; ++w) t += red[w][threadIdx.x];
        if (t != 0u) atomicAdd(&rec[threadIdx.x], (unsigned long long)t);
    }
}

// ---------------------------------------------------------------- host side
u64 setop_tiles(u64 n) { return ceil_div(n, SETOP_TILE); }
size_t setop_split_bytes(u64 n) { return align256(16u * (setop_tiles(n) + 1u)); }

// f(std::integral_constant<u32, op>{}): the one place `op` becomes the OP of the count and the write kernel
template <typename F>
void with_op(u32 op, F&& f) {
    switch (op) {
        case KMX_SETOP_INTERSECT: return f(std::integral_constant<u32, KMX_SETOP_INTERSECT>{});
        case KMX_SETOP_UNION: return f(std::integral_constant<u32, KMX_SETOP_UNION>{});
        case KMX_SETOP_SUBTRACT: return f(std::integral_constant<u32, KMX_SETOP_SUBTRACT>{});
        case KMX_SETOP_SYMDIFF: return f(std::integral_constant<u32, KMX_SETOP_SYMDIFF>{});
        default: return f(std::integral_constant<u32, KMX_SETOP_COUNTER_SUBTRACT>{});
    }
}

template <u32 W>
void partition(const u64* ka, u64 na, const u64* kb, u64 nb, u64* split, hipStream_t st) {
    const u64 nt = setop_tiles(na + nb);
    hipLaunchKernelGGL(setop_partition_kernel<W>, dim3((unsigned)ceil_div(nt + 1u, CT)), dim3(CT), 0, st, ka, na, kb, nb, nt, split);
}

}  // namespace

// The working set of a set operation or a comparison of n = n_a + n_b entries: two u64 per cut (tiles + 1 cuts) and one u64 per
// tile + 2 (the totals, their sum; the comparison's record), each array rounded up to 256 bytes.
size_t count_setop_bytes(u64 n) { return setop_split_bytes(n) + align256(8u * (setop_tiles(n) + 2u)); }

// partition, count pass, scan; synchronous (one host round trip: the size of the result).  na + nb > 0.
hipError_t launch_count_setop(u32 words, u32 op, const u64* ka, const u64* ca, u64 na, const u64* kb, const u64* cb, u64 nb, void* area,
                              unsigned long long* h_pinned, u64* h_out, hipStream_t st) {
    u64* split = static_cast<u64*>(area);
    u64* partial = reinterpret_cast<u64*>(static_cast<char*>(area) + setop_split_bytes(na + nb));
    const u64 nt = setop_tiles(na + nb);
    with_width(words, [&](auto w) {
        constexpr u32 W = decltype(w)::value;
        partition<W>(ka, na, kb, nb, split, st);
        with_op(op, [&](auto o) {
            hipLaunchKernelGGL((setop_count_kernel<W, decltype(o)::value>), dim3((unsigned)nt), dim3(CT), 0, st, ka, ca, kb, cb, split, partial);
        });
    });
    hipLaunchKernelGGL(scan_single_kernel, dim3(1), dim3(CT), 0, st, partial, nt, partial + nt);
    return read_back(h_pinned, partial + nt, 1u, h_out, st);
}

hipError_t launch_count_setop_emit(u32 words, u32 op, u32 rule, const u64* ka, const u64* ca, u64 na, const u64* kb, const u64* cb, u64 nb,
                                   const void* area, u64* out_k, u64* out_c, hipStream_t st) {
    const u64* split = static_cast<const u64*>(area);
    const u64* partial = reinterpret_cast<const u64*>(static_cast<const char*>(area) + setop_split_bytes(na + nb));
    const unsigned nt = (unsigned)setop_tiles(na + nb);
    with_width(words, [&](auto w) {
        with_op(op, [&](auto o) {
            hipLaunchKernelGGL((setop_write_kernel<decltype(w)::value, decltype(o)::value>), dim3(nt), dim3(CT), 0, st, ka, ca, kb, cb, split, partial,
                               rule, out_k, out_c);
        });
    });
    return hipGetLastError();
}

// h_rec[0 .. 6) = n_both, sum_a, sum_b, sum_a_both, sum_b_both, sum_min; synchronous (one host round trip: the record)
hipError_t launch_count_compare(u32 words, const u64* ka, const u64* ca, u64 na, const u64* kb, const u64* cb, u64 nb, void* area,
                                unsigned long long* h_pinned, u64* h_rec, hipStream_t st) {
    u64* split = static_cast<u64*>(area);
    unsigned long long* rec = reinterpret_cast<unsigned long long*>(static_cast<char*>(area) + setop_split_bytes(na + nb));
    const unsigned nt = (unsigned)setop_tiles(na + nb);
    hipError_t e = hipMemsetAsync(rec, 0, 8u * CMP_WORDS, st);
    if (e != hipSuccess) return e;
    with_width(words, [&](auto w) {
        partition<decltype(w)::value>(ka, na, kb, nb, split, st);
        hipLaunchKernelGGL(setop_compare_kernel<decltype(w)::value>, dim3(nt), dim3(CT), 0, st, ka, ca, kb, cb, split, rec);
    });
    return read_back(h_pinned, rec, CMP_WORDS, h_rec, st);
}

}  // namespace kmx
