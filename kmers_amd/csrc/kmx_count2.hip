// kmx_count2.hip -- exact canonical k-mer counting for two-word k-mers, k = 33..64 (kmx_count_canonical2), and the union of two
// such tables (kmx_count_merge2).  The structure is that of kmx_count.hip and is described there: MSD radix partition on the
// key's own bits, 8 per level from bit 2k down (count -> column scan -> per-partition finalise -> scatter), small children
// gathered into leaf groups that a block sorts in LDS and run-length encodes, runs marked by a byte and compacted at the end,
// one host round trip per level.  What a 16-byte key changes:
//   - a key is one 16-byte element {lo, hi} everywhere (the slot layout of kmx_canonical_windows2): one dwordx4 access per lane in
//     global memory, one b128 element in LDS; the order is the 2k-bit integer's -- high word first, then low;
//   - a digit is bits [hi_bit - 8, hi_bit) of the 128-bit value and may straddle the two words (2k mod 8 != 0);
//   - "every key of the partition is equal" has no 64-bit min / max to lean on: a thread compares its keys with the first one it
//     met, a tile leaves {a key of its own, has keys, keys differ} in a record per tile, and the partition's finalise block folds
//     its tiles' records the same way.  No atomic on global memory, no order between blocks; an all-A batch still costs the
//     window pass and one count pass;
//   - a run's count goes into the low word of the same slot of the other array (the one-word scheme with 16-byte slots).
// Leaf capacities: a group of up to LEAF_SMALL = 512 keys takes 8 KiB of keys (11 KiB of LDS a block: eight blocks, the CU's 32
// waves); a child of 513..4096 keys takes 64 KiB (74 KiB a block: two blocks per CU).  The large capacity is kept at 4096 because
// the partition arrays -- 2 KiB of digit totals per partition -- are bounded by n / (LEAF + 1) partitions: at 2048 they alone
// would take another byte per window, and on random reads nearly every key reaches a leaf through the small groups.
// Bitonic strides of 16 elements and more read and write consecutive 16-byte elements per lane group (conflict-free); strides
// 1, 2, 4, 8 are two-way conflicts on the b128 lane groups, exactly what the 8-byte layout of kmx_count.hip pays at the same
// strides -- a lo plane / hi plane layout has the same pattern at twice the instructions, so the element layout stays.
#include "kmx_count_common.h"

namespace kmx {

namespace {

constexpr u32 TILE = 16384;                   // keys per block in the partition passes
constexpr u32 LEAF = 4096;                    // keys a leaf block sorts in LDS (64 KiB of keys)
constexpr u32 LEAF_SMALL = 512;               // leaf groups are gathered up to this size (8 KiB of keys)

struct alignas(16) K2 {
    u64 lo, hi;
};
static_assert(sizeof(K2) == 16, "a key is one 16-byte element");

__device__ __forceinline__ bool k2_ne(const K2& a, const K2& b) { return ((a.lo ^ b.lo) | (a.hi ^ b.hi)) != 0; }
__device__ __forceinline__ bool k2_lt(const K2& a, const K2& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
// bits [sh, sh + 8) of the key (the caller masks): sh is uniform over the block
__device__ __forceinline__ u32 k2_bits(const K2& key, u32 sh) {
    if (sh >= 64u) return (u32)(key.hi >> (sh - 64u));
    if (sh == 0u) return (u32)key.lo;
    return (u32)((key.lo >> sh) | (key.hi << (64u - sh)));
}

struct Seg2 {
    u64 start;      // first index of the partition (output coordinates; level 0: the window array)
    u64 n;          // keys (level 0: windows, valid or not)
    u64 tile_base;  // first tile of the partition in this level's tile space
    u32 hi_bit;     // bits not yet partitioned: the digit is bits [hi_bit - w, hi_bit), w = min(8, hi_bit)
    u32 skip;       // segfinal wrote the partition's runs itself: no scatter
};

// what a tile's count pass says about its keys (a record per tile of the level)
struct TileKeys {
    K2 ref;         // one of the tile's keys (if it has any)
    u32 state;      // SAME_HAS: the tile holds a key; SAME_DIFF: not all of them equal `ref`
    u32 pad[3];
};
constexpr u32 SAME_HAS = 1u, SAME_DIFF = 2u;

// Fold of (has, one key, differs) over the block: every thread brings what it saw; on return sm->state and sm->ref hold the
// block's.  The reference is the key of the lowest thread that has one, so the result does not depend on timing.
struct SameKeys {
    K2 ref;
    u32 first, state;
};
__device__ __forceinline__ void same_init(SameKeys* sm) {
    if (threadIdx.x == 0) {
        sm->first = CT;
        sm->state = 0u;
    }
}
// (a barrier lies between same_init and this)
__device__ __forceinline__ void same_fold(SameKeys* sm, bool has, const K2& f, bool diff) {
    if (has) atomicMin(&sm->first, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == sm->first) {
        sm->ref = f;
        sm->state = SAME_HAS;
    }
    __syncthreads();
    if (has && (diff || k2_ne(f, sm->ref))) atomicOr(&sm->state, SAME_DIFF);
    __syncthreads();
}

// ---------------------------------------------------------------- one level of the partition
__device__ __forceinline__ void tile_range(const Seg2& s, u64 t_local, u64* lo, u64* hi) {
    *lo = s.start + t_local * TILE;
    const u64 e = *lo + TILE, end = s.start + s.n;
    *hi = e < end ? e : end;
}

// L0: the input is the window array (canon2 + flags, invalid windows dropped); above: the keys of the partitions
template <bool L0>
__global__ void __launch_bounds__(CT) count2_kernel(const Seg2* __restrict__ segs, const u32* __restrict__ tile_seg, const K2* __restrict__ in,
                                                    const uint8_t* __restrict__ flags, u64* __restrict__ hist, TileKeys* __restrict__ tkeys) {
    __shared__ u32 h[RADIX];
    __shared__ SameKeys sm;
    const u32 si = L0 ? 0u : tile_seg[blockIdx.x];
    const Seg2 s = segs[si];
    const u64 t_local = blockIdx.x - s.tile_base, nt = ceil_div(s.n, TILE);
    const u32 w = digit_width(s.hi_bit), sh = s.hi_bit - w, mask = (1u << w) - 1u;
    h[threadIdx.x] = 0;
    same_init(&sm);
    __syncthreads();
    u64 lo, hi;
    tile_range(s, t_local, &lo, &hi);
    bool has = false, diff = false;
    K2 f{0u, 0u};
    for (u64 i = lo + threadIdx.x; i < hi; i += CT) {
        if (L0 && !(flags[i] & KMX_WIN_VALID)) continue;
        const K2 key = in[i];
        atomicAdd(&h[k2_bits(key, sh) & mask], 1u);
        if (!has) {
            f = key;
            has = true;
        } else {
            diff |= k2_ne(key, f);
        }
    }
    same_fold(&sm, has, f, diff);   // (its barriers also close the histogram)
    hist[s.tile_base * RADIX + (u64)threadIdx.x * nt + t_local] = h[threadIdx.x];
    if (threadIdx.x == 0) tkeys[blockIdx.x] = TileKeys{sm.ref, sm.state, {0u, 0u, 0u}};
}

// a block per (partition, digit): the digit's per-tile counts -> exclusive prefix; the digit's total -> coltot.  Level 0: its one
// partition; above: the partitions of more than COL_SERIAL tiles, listed in `big`
__global__ void __launch_bounds__(CT) colscan2_kernel(const Seg2* __restrict__ segs, const u32* __restrict__ big, u64* __restrict__ hist,
                                                      u64* __restrict__ coltot) {
    __shared__ u64 sh[CT];
    const u32 si = big ? big[blockIdx.x / RADIX] : blockIdx.x / RADIX, b = blockIdx.x % RADIX;
    const Seg2 s = segs[si];
    const u64 nt = ceil_div(s.n, TILE);
    u64 tot;
    block_scan_array(hist + s.tile_base * RADIX + (u64)b * nt, nt, sh, &tot);
    if (threadIdx.x == 0) coltot[(u64)si * RADIX + b] = tot;
}

// levels above 0: a block per partition of at most COL_SERIAL tiles, a thread per digit walking its column (longer ones: above)
__global__ void __launch_bounds__(CT) colscan2_seg_kernel(const Seg2* __restrict__ segs, u64* __restrict__ hist, u64* __restrict__ coltot) {
    const Seg2 s = segs[blockIdx.x];
    const u64 nt = ceil_div(s.n, TILE);
    u64* h = hist + s.tile_base * RADIX;
    if (nt <= COL_SERIAL) {
        u64* c = h + (u64)threadIdx.x * nt;
        u64 run = 0;
        for (u64 t = 0; t < nt; ++t) {
            const u64 v = c[t];
            c[t] = run;
            run += v;
        }
        coltot[(u64)blockIdx.x * RADIX + threadIdx.x] = run;
    }
}

// a block per partition: the digit totals -> the children's bases (in coltot, relative to the partition's start); the tiles'
// records -> "one key"; the partition's runs if it needs no scatter; else its children to the next level and the leaf groups
__global__ void __launch_bounds__(CT) segfinal2_kernel(Seg2* __restrict__ segs, u64* __restrict__ coltot, const TileKeys* __restrict__ tkeys,
                                                       Seg2* __restrict__ next, u64 max_next, u32* __restrict__ big, u64 max_big,
                                                       Leaf* __restrict__ leaves, u64 max_leaf, Leaf* __restrict__ small, u64 max_small,
                                                       Counters* __restrict__ cnt, u32 dst_is_keys,
                                                       K2* __restrict__ keys, K2* __restrict__ other, uint8_t* __restrict__ keep, u32 level0) {
    __shared__ u64 sh[CT];
    __shared__ SameKeys sm;
    const u32 si = blockIdx.x;
    const Seg2 s = segs[si];
    same_init(&sm);
    const u64 v = coltot[(u64)si * RADIX + threadIdx.x];
    u64 total;
    const u64 base = block_exscan(v, sh, &total);
    coltot[(u64)si * RADIX + threadIdx.x] = base;
    if (level0 && threadIdx.x == 0) cnt->n_valid = total;
    if (total == 0) {
        if (threadIdx.x == 0) segs[si].skip = 1u;
        return;
    }
    {   // the tiles' records, folded as a tile folds its keys
        const u64 nt = ceil_div(s.n, TILE);
        bool has = false, diff = false;
        K2 f{0u, 0u};
        for (u64 t = threadIdx.x; t < nt; t += CT) {
            const TileKeys tk = tkeys[s.tile_base + t];
            if (!(tk.state & SAME_HAS)) continue;
            diff |= (tk.state & SAME_DIFF) != 0;
            if (!has) {
                f = tk.ref;
                has = true;
            } else {
                diff |= k2_ne(tk.ref, f);
            }
        }
        same_fold(&sm, has, f, diff);
    }
    const K2 ref = sm.ref;
    const u32 w = digit_width(s.hi_bit), shift = s.hi_bit - w;
    if (!(sm.state & SAME_DIFF)) {   // one key: one run
        if (threadIdx.x == 0) {
            keys[s.start] = ref;
            other[s.start] = K2{total, 0u};
            keep[s.start] = 1u;
            segs[si].skip = 1u;
        }
        return;
    }
    if (shift == 0) {     // the last digit: every bucket is one key (the bits above it are the partition's own)
        if (v != 0) {
            keys[s.start + base] = K2{((ref.lo >> w) << w) | threadIdx.x, ref.hi};
            other[s.start + base] = K2{v, 0u};
            keep[s.start + base] = 1u;
        }
        if (threadIdx.x == 0) segs[si].skip = 1u;
        return;
    }
    // (sh[] holds the inclusive scan of the totals until the next barrier: keep the bases in a table of their own)
    __shared__ u64 bases[RADIX];
    bases[threadIdx.x] = base;
    __syncthreads();
    if (threadIdx.x != 0) return;
    segs[si].skip = 0u;
    // two walks over the children: the first counts what this partition adds to each list (one atomic per list and partition
    // then reserves the slots), the second writes
    unsigned long long n_small = 0, n_big = 0, n_nx = 0, n_nx_tiles = 0;
    for (int pass = 0; pass < 2; ++pass) {
        unsigned long long i_small = 0, i_big = 0, i_nx = 0, i_tile = 0;
        if (pass == 1) {
            i_small = n_small ? atomicAdd(&cnt->n_leaf_small, n_small) : 0ull;
            i_big = n_big ? atomicAdd(&cnt->n_leaf, n_big) : 0ull;
            i_nx = n_nx ? atomicAdd(&cnt->n_next, n_nx) : 0ull;
            i_tile = n_nx ? atomicAdd(&cnt->n_next_tiles, n_nx_tiles) : 0ull;
            if (i_small + n_small > max_small || i_big + n_big > max_leaf || i_nx + n_nx > max_next) {
                atomicOr(&cnt->overflow, 1ull);
                return;
            }
        }
        u64 g_start = 0, g_n = 0;
        auto flush = [&]() {
            if (g_n == 0) return;
            if (pass == 1) small[i_small] = Leaf{g_start, g_n, dst_is_keys, 0u};
            ++i_small;
            g_n = 0;
        };
        for (u32 b = 0; b < RADIX; ++b) {
            const u64 nb = (b + 1u < RADIX ? bases[b + 1u] : total) - bases[b];
            if (nb == 0) continue;
            const u64 sb = s.start + bases[b];
            if (nb > LEAF) {
                flush();
                const u64 nt = ceil_div(nb, TILE);
                if (pass == 1) {
                    next[i_nx] = Seg2{sb, nb, i_tile, shift, 0u};
                    if (nt > COL_SERIAL) {   // (rare: more than COL_SERIAL * TILE keys)
                        const unsigned long long bi = atomicAdd(&cnt->n_next_big, 1ull);
                        if (bi < max_big) big[bi] = (u32)i_nx;
                        else atomicOr(&cnt->overflow, 1ull);
                    }
                }
                ++i_nx;
                i_tile += nt;
            } else if (nb > LEAF_SMALL) {   // a leaf of its own on the large network
                flush();
                if (pass == 1) leaves[i_big] = Leaf{sb, nb, dst_is_keys, 0u};
                ++i_big;
            } else {
                if (g_n + nb > LEAF_SMALL) flush();
                if (g_n == 0) g_start = sb;
                g_n += nb;
            }
        }
        flush();
        if (pass == 0) {
            n_small = i_small;
            n_big = i_big;
            n_nx = i_nx;
            n_nx_tiles = i_tile;
        }
    }
}

template <bool L0>
__global__ void __launch_bounds__(CT) scatter2_kernel(const Seg2* __restrict__ segs, const u32* __restrict__ tile_seg, const K2* __restrict__ in,
                                                      const uint8_t* __restrict__ flags, const u64* __restrict__ hist,
                                                      const u64* __restrict__ coltot, K2* __restrict__ out) {
    __shared__ u64 pos[RADIX];
    __shared__ u32 fill[RADIX];
    const u32 si = L0 ? 0u : tile_seg[blockIdx.x];
    const Seg2 s = segs[si];
    if (s.skip) return;
    const u64 t_local = blockIdx.x - s.tile_base, nt = ceil_div(s.n, TILE);
    const u32 w = digit_width(s.hi_bit), sh = s.hi_bit - w, mask = (1u << w) - 1u;
    // (level 0: the window array is indexed from 0 and the keys land in [0, n_valid): its start is 0 in both)
    pos[threadIdx.x] = s.start + coltot[(u64)si * RADIX + threadIdx.x] + hist[s.tile_base * RADIX + (u64)threadIdx.x * nt + t_local];
    fill[threadIdx.x] = 0;
    __syncthreads();
    u64 lo, hi;
    tile_range(s, t_local, &lo, &hi);
    for (u64 i = lo + threadIdx.x; i < hi; i += CT) {
        if (L0 && !(flags[i] & KMX_WIN_VALID)) continue;
        const K2 key = in[i];
        const u32 d = k2_bits(key, sh) & mask;
        out[pos[d] + atomicAdd(&fill[d], 1u)] = key;
    }
}

// level 0: one partition, the whole window array
__global__ void seg2_init_kernel(Seg2* __restrict__ segs, u64 n_win, u32 hi_bit) { segs[0] = Seg2{0u, n_win, 0u, hi_bit, 0u}; }

// the tiles of the next level's partitions -> their partition
__global__ void __launch_bounds__(CT) tilemap2_kernel(const Seg2* __restrict__ segs, u32* __restrict__ tile_seg) {
    const Seg2 s = segs[blockIdx.x];
    const u64 nt = ceil_div(s.n, TILE);
    for (u64 j = threadIdx.x; j < nt; j += CT) tile_seg[s.tile_base + j] = blockIdx.x;
}

// a block per leaf group of at most CAP keys: bitonic sort in LDS (a key is one 16-byte element), run-length encoding
template <u32 CAP>
__global__ void __launch_bounds__(CT) leaf2_kernel(const Leaf* __restrict__ leaves, K2* __restrict__ keys, K2* __restrict__ other,
                                                   uint8_t* __restrict__ keep) {
    __shared__ K2 a[CAP];
    __shared__ uint16_t head_at[CAP];
    __shared__ u64 sh[CT];
    const Leaf L = leaves[blockIdx.x];
    const u32 n = (u32)L.n;
    const K2* src = L.in_keys ? keys : other;
    u32 P = 2;
    while (P < n) P <<= 1;
    for (u32 i = threadIdx.x; i < P; i += CT) a[i] = i < n ? src[L.start + i] : K2{~0ull, ~0ull};
    for (u32 size = 2; size <= P; size <<= 1) {
        for (u32 stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (u32 t = threadIdx.x; t < (P >> 1); t += CT) {
                const u32 i = 2u * t - (t & (stride - 1u)), j = i + stride;
                const bool up = (i & size) == 0;
                const K2 x = a[i], y = a[j];
                if (k2_lt(y, x) == up) {
                    a[i] = y;
                    a[j] = x;
                }
            }
        }
    }
    __syncthreads();
    // run heads: thread t looks at positions [PER t, PER t + PER)
    constexpr u32 PER = CAP / CT;
    const u32 i0 = threadIdx.x * PER;
    u32 heads = 0;
    for (u32 j = 0; j < PER; ++j) {
        const u32 i = i0 + j;
        if (i < n && (i == 0 || k2_ne(a[i], a[i - 1u]))) ++heads;
    }
    u64 nd;
    u32 r = (u32)block_exscan(heads, sh, &nd);
    for (u32 j = 0; j < PER; ++j) {
        const u32 i = i0 + j;
        if (i < n && (i == 0 || k2_ne(a[i], a[i - 1u]))) head_at[r++] = (uint16_t)i;
    }
    __syncthreads();
    for (u32 q = threadIdx.x; q < (u32)nd; q += CT) {
        const u32 p = head_at[q], e = q + 1u < (u32)nd ? (u32)head_at[q + 1u] : n;
        keys[L.start + q] = a[p];
        other[L.start + q] = K2{(u64)(e - p), 0u};
        keep[L.start + q] = 1u;
    }
}

// ---------------------------------------------------------------- compaction of the kept entries
// a wave per quarter of the block's positions, 64 at a time: the ballot of the kept bytes gives each lane its slot
__global__ void __launch_bounds__(CT) keep_write2_kernel(const uint8_t* __restrict__ keep, const u64* __restrict__ partial, const K2* __restrict__ keys,
                                                         const K2* __restrict__ counts, K2* __restrict__ out_k, u64* __restrict__ out_c) {
    constexpr u32 PER_WAVE = CHUNK / (CT / 64u);
    static_assert(PER_WAVE == 64u * 64u, "a wave's range is its lanes' 64-byte pieces");
    __shared__ u32 wsum[CT / 64];
    const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const u64 w0 = (u64)blockIdx.x * CHUNK + (u64)wv * PER_WAVE;
    u32 c = kept_in(keep, w0 + (u64)lane * 64u);
    for (u32 o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) wsum[wv] = c;
    __syncthreads();
    u64 o = partial[blockIdx.x];
    for (u32 j = 0; j < wv; ++j) o += wsum[j];
    for (u32 s0 = 0; s0 < PER_WAVE; s0 += 64u) {
        const u64 i = w0 + s0 + lane;
        const bool kp = keep[i] != 0;
        const unsigned long long m = __ballot(kp);
        if (kp) {
            const u64 r = o + (u64)__popcll(m & ((1ull << lane) - 1ull));
            out_k[r] = keys[i];
            out_c[r] = counts[i].lo;
        }
        o += (u64)__popcll(m);
    }
}

// ---------------------------------------------------------------- merge of two tables
// merge path: thread t writes outputs [8 t, 8 t + 8); on equal keys the item of `a` goes first
__global__ void __launch_bounds__(CT) merge2_kernel(const K2* __restrict__ ka, const u64* __restrict__ ca, u64 na, const K2* __restrict__ kb,
                                                    const u64* __restrict__ cb, u64 nb, K2* __restrict__ mk, u64* __restrict__ mc) {
    const u64 n = na + nb, d = ((u64)blockIdx.x * CT + threadIdx.x) * MERGE_IPT;
    if (d >= n) return;
    u64 lo = d > nb ? d - nb : 0u, hi = d < na ? d : na;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (!k2_lt(kb[d - 1u - mid], ka[mid])) lo = mid + 1u;
        else hi = mid;
    }
    u64 i = lo, j = d - lo;
    for (u32 q = 0; q < MERGE_IPT && d + q < n; ++q) {
        bool take_a = j >= nb;
        K2 x{0u, 0u}, y{0u, 0u};
        if (i < na) x = ka[i];
        if (j < nb) y = kb[j];
        if (!take_a && i < na) take_a = !k2_lt(y, x);
        if (take_a) {
            mk[d + q] = x;
            mc[d + q] = ca[i];
            ++i;
        } else {
            mk[d + q] = y;
            mc[d + q] = cb[j];
            ++j;
        }
    }
}

__device__ __forceinline__ bool is_head2(const K2* mk, u64 i) { return i == 0 || k2_ne(mk[i], mk[i - 1u]); }

__global__ void __launch_bounds__(CT) head_count2_kernel(const K2* __restrict__ mk, u64 n, u64* __restrict__ partial) {
    __shared__ u64 sh[CT];
    const u64 i0 = (u64)blockIdx.x * MCHUNK + (u64)threadIdx.x * 16u;
    u64 c = 0;
    for (u32 j = 0; j < 16; ++j)
        if (i0 + j < n && is_head2(mk, i0 + j)) ++c;
    u64 tot;
    (void)block_exscan(c, sh, &tot);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(CT) head_write2_kernel(const K2* __restrict__ mk, const u64* __restrict__ mc, u64 n, const u64* __restrict__ partial,
                                                         K2* __restrict__ out_k, u64* __restrict__ out_c) {
    __shared__ u64 sh[CT];
    const u64 i0 = (u64)blockIdx.x * MCHUNK + (u64)threadIdx.x * 16u;
    u64 c = 0;
    for (u32 j = 0; j < 16; ++j)
        if (i0 + j < n && is_head2(mk, i0 + j)) ++c;
    u64 tot;
    u64 o = partial[blockIdx.x] + block_exscan(c, sh, &tot);
    for (u32 j = 0; j < 16; ++j) {
        const u64 i = i0 + j;
        if (i < n && is_head2(mk, i)) {
            // (each table holds a key once: an equal neighbour is the other table's entry)
            out_k[o] = mk[i];
            out_c[o] = mc[i] + (i + 1u < n && !k2_ne(mk[i + 1u], mk[i]) ? mc[i + 1u] : 0u);
            ++o;
        }
    }
}

// bounds of one level's arrays for n keys (kmx_count.hip says why these hold)
u64 max_segs(u64 n) { return n / (LEAF + 1u) + 2u; }
u64 max_tiles(u64 n) { return ceil_div(n, TILE) + max_segs(n) + 1u; }
u64 max_big(u64 n) { return ceil_div(n, (u64)COL_SERIAL * TILE) + 2u; }   // partitions of more than COL_SERIAL tiles
u64 max_leaves(u64 n) { return ceil_div(n, LEAF_SMALL + 1u) + 64u; }
u64 max_small_leaves(u64 n) { return 3u * ceil_div(n, LEAF_SMALL + 1u) + max_segs(n) + 64u; }

// ---------------------------------------------------------------- host side
// The work area of one count, after the canon2 / flags arrays: keys (16 B per window), keep (1 B per window), then the
// level arrays (~1.35 B per window: 2 KiB of tile histograms per tile and of digit bases per partition, the leaf lists).
// `n` = the windows the area is sized for.
struct CountArea2 {
    K2* keys;
    uint8_t* keep;
    u64* hist;
    u64* coltot;
    u32* tile_seg;
    u32* big;
    TileKeys* tkeys;
    Seg2* segs[2];
    Leaf* leaves;
    Leaf* small;
    u64* partial;
    Counters* cnt;
    size_t keep_bytes;
};

size_t area_layout(u64 n, CountArea2* out, void* base) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += align256(bytes);
        return base ? static_cast<char*>(base) + at : nullptr;
    };
    CountArea2 a{};
    a.keys = reinterpret_cast<K2*>(take(16u * n));
    a.keep_bytes = ceil_div(n, CHUNK) * CHUNK;
    a.keep = reinterpret_cast<uint8_t*>(take(a.keep_bytes));
    a.hist = reinterpret_cast<u64*>(take(8u * RADIX * max_tiles(n)));
    a.coltot = reinterpret_cast<u64*>(take(8u * RADIX * max_segs(n)));
    a.tile_seg = reinterpret_cast<u32*>(take(4u * max_tiles(n)));
    a.big = reinterpret_cast<u32*>(take(4u * max_big(n)));
    a.tkeys = reinterpret_cast<TileKeys*>(take(sizeof(TileKeys) * max_tiles(n)));
    a.segs[0] = reinterpret_cast<Seg2*>(take(sizeof(Seg2) * max_segs(n)));
    a.segs[1] = reinterpret_cast<Seg2*>(take(sizeof(Seg2) * max_segs(n)));
    a.leaves = reinterpret_cast<Leaf*>(take(sizeof(Leaf) * max_leaves(n)));
    a.small = reinterpret_cast<Leaf*>(take(sizeof(Leaf) * max_small_leaves(n)));
    a.partial = reinterpret_cast<u64*>(take(8u * (ceil_div(n, CHUNK) + 2u)));
    a.cnt = reinterpret_cast<Counters*>(take(sizeof(Counters)));
    if (out) *out = a;
    return off;
}

}  // namespace

size_t count2_area_bytes(u64 n) { return area_layout(n, nullptr, nullptr); }

// Sort and tally the n_win windows (canon2: 2 u64 per window, 16-byte aligned; flags) of a batch of two-word k-mers; the table is
// left in `area` (keys in a.keys, counts in the low words of canon2's slots, marked in a.keep) and its size comes back in
// *h_distinct.  Synchronous: one host round trip per level and one for the number of distinct keys.  *bad: the level arrays
// overflowed their bounds (a bug, never expected).
hipError_t launch_count2_sort(u64* canon2, const uint8_t* flags, u64 n_win, u32 k, void* area, unsigned long long* h_pinned, u64* h_valid,
                              u64* h_distinct, bool* bad, hipStream_t st) {
    CountArea2 a;
    area_layout(n_win, &a, area);
    K2* canon = reinterpret_cast<K2*>(canon2);
    *bad = false;
    hipError_t e;
    if ((e = hipMemsetAsync(a.keep, 0, a.keep_bytes, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(seg2_init_kernel, dim3(1), dim3(1), 0, st, a.segs[0], n_win, 2u * k);
    const u64 ms = max_segs(n_win), ml = max_leaves(n_win), mls = max_small_leaves(n_win), mt = max_tiles(n_win), mb = max_big(n_win);
    u64 n_seg = 1, n_tiles = ceil_div(n_win, TILE), n_big = 0;
    *h_valid = 0;
    for (u32 level = 0; n_seg != 0; ++level) {
        if (level > 16u) {   // (2k <= 128 bits: at most 16 digits)
            *bad = true;
            return hipSuccess;
        }
        const bool l0 = level == 0;
        Seg2* cur = a.segs[level & 1u];
        Seg2* nxt = a.segs[(level & 1u) ^ 1u];
        // level 0 reads the windows (canon2) and writes `keys`; then the levels alternate
        const bool src_is_keys = (level & 1u) == 1u;
        K2* src = src_is_keys ? a.keys : canon;
        K2* dst = src_is_keys ? canon : a.keys;
        if ((e = hipMemsetAsync(a.cnt, 0, LEVEL_COUNTERS, st)) != hipSuccess) return e;
        if (l0) hipLaunchKernelGGL(count2_kernel<true>, dim3((unsigned)n_tiles), dim3(CT), 0, st, cur, a.tile_seg, src, flags, a.hist, a.tkeys);
        else hipLaunchKernelGGL(count2_kernel<false>, dim3((unsigned)n_tiles), dim3(CT), 0, st, cur, a.tile_seg, src, flags, a.hist, a.tkeys);
        if (l0) {
            hipLaunchKernelGGL(colscan2_kernel, dim3(RADIX), dim3(CT), 0, st, cur, (const u32*)nullptr, a.hist, a.coltot);
        } else {
            hipLaunchKernelGGL(colscan2_seg_kernel, dim3((unsigned)n_seg), dim3(CT), 0, st, cur, a.hist, a.coltot);
            if (n_big) hipLaunchKernelGGL(colscan2_kernel, dim3((unsigned)(n_big * RADIX)), dim3(CT), 0, st, cur, (const u32*)a.big, a.hist, a.coltot);
        }
        hipLaunchKernelGGL(segfinal2_kernel, dim3((unsigned)n_seg), dim3(CT), 0, st, cur, a.coltot, a.tkeys, nxt, ms, a.big, mb, a.leaves, ml, a.small, mls,
                           a.cnt, src_is_keys ? 0u : 1u, a.keys, canon, a.keep, l0 ? 1u : 0u);
        if (l0) hipLaunchKernelGGL(scatter2_kernel<true>, dim3((unsigned)n_tiles), dim3(CT), 0, st, cur, a.tile_seg, src, flags, a.hist, a.coltot, dst);
        else hipLaunchKernelGGL(scatter2_kernel<false>, dim3((unsigned)n_tiles), dim3(CT), 0, st, cur, a.tile_seg, src, flags, a.hist, a.coltot, dst);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(h_pinned, a.cnt, LEVEL_COUNTERS, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
        if (l0) *h_valid = h_pinned[0];
        const u64 n_next = h_pinned[1], n_next_tiles = h_pinned[2], n_leaf = h_pinned[3], n_small = h_pinned[5], n_next_big = h_pinned[6];
        if (h_pinned[4] != 0 || n_next > ms || n_leaf > ml || n_small > mls || n_next_tiles > mt || n_next_big > mb) {
            *bad = true;
            return hipSuccess;
        }
        if (n_leaf) hipLaunchKernelGGL(leaf2_kernel<LEAF>, dim3((unsigned)n_leaf), dim3(CT), 0, st, a.leaves, a.keys, canon, a.keep);
        if (n_small) hipLaunchKernelGGL(leaf2_kernel<LEAF_SMALL>, dim3((unsigned)n_small), dim3(CT), 0, st, a.small, a.keys, canon, a.keep);
        if (n_next) hipLaunchKernelGGL(tilemap2_kernel, dim3((unsigned)n_next), dim3(CT), 0, st, nxt, a.tile_seg);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        n_seg = n_next;
        n_tiles = n_next_tiles;
        n_big = n_next_big;
    }
    const u64 nb = ceil_div(*h_valid, CHUNK);
    *h_distinct = 0;
    if (nb == 0) return hipSuccess;
    hipLaunchKernelGGL(keep_count_kernel, dim3((unsigned)nb), dim3(CT), 0, st, a.keep, a.partial);
    hipLaunchKernelGGL(scan_single_kernel, dim3(1), dim3(CT), 0, st, a.partial, nb, &a.cnt->n_distinct);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(h_pinned, &a.cnt->n_distinct, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    *h_distinct = h_pinned[0];
    return hipSuccess;
}

// the table launch_count2_sort left in `area` -> out_k2 (2 u64 per entry) / out_c (n_distinct entries)
hipError_t launch_count2_emit(const u64* canon2, u64 n_win, u64 n_valid, void* area, u64* out_k2, u64* out_c, hipStream_t st) {
    CountArea2 a;
    area_layout(n_win, &a, area);
    const u64 nb = ceil_div(n_valid, CHUNK);
    if (nb)
        hipLaunchKernelGGL(keep_write2_kernel, dim3((unsigned)nb), dim3(CT), 0, st, a.keep, a.partial, a.keys, reinterpret_cast<const K2*>(canon2),
                           reinterpret_cast<K2*>(out_k2), out_c);
    return hipGetLastError();
}

// merged keys (16 B per input entry), their counts (8 B), the blocks' head counts
size_t count2_merge_bytes(u64 n) { return align256(16u * n) + align256(8u * n) + align256(8u * (ceil_div(n, MCHUNK) + 2u)); }

// merge of two tables into `area` and the number of distinct keys of the union (synchronous: one host round trip)
hipError_t launch_count2_merge(const u64* ka, const u64* ca, u64 na, const u64* kb, const u64* cb, u64 nb, void* area, unsigned long long* h_pinned,
                               u64* h_out, hipStream_t st) {
    const u64 n = na + nb;
    K2* mk = static_cast<K2*>(area);
    u64* mc = reinterpret_cast<u64*>(static_cast<char*>(area) + align256(16u * n));
    u64* partial = reinterpret_cast<u64*>(static_cast<char*>(area) + align256(16u * n) + align256(8u * n));
    const u64 nblk = ceil_div(n, MCHUNK);
    hipLaunchKernelGGL(merge2_kernel, dim3((unsigned)ceil_div(n, (u64)CT * MERGE_IPT)), dim3(CT), 0, st, reinterpret_cast<const K2*>(ka), ca, na,
                       reinterpret_cast<const K2*>(kb), cb, nb, mk, mc);
    hipLaunchKernelGGL(head_count2_kernel, dim3((unsigned)nblk), dim3(CT), 0, st, (const K2*)mk, n, partial);
    hipLaunchKernelGGL(scan_single_kernel, dim3(1), dim3(CT), 0, st, partial, nblk, partial + nblk);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = hipMemcpyAsync(h_pinned, partial + nblk, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    *h_out = h_pinned[0];
    return hipSuccess;
}

hipError_t launch_count2_merge_emit(u64 n, const void* area, u64* out_k2, u64* out_c, hipStream_t st) {
    const K2* mk = static_cast<const K2*>(area);
    const u64* mc = reinterpret_cast<const u64*>(static_cast<const char*>(area) + align256(16u * n));
    const u64* partial = reinterpret_cast<const u64*>(static_cast<const char*>(area) + align256(16u * n) + align256(8u * n));
    const u64 nblk = ceil_div(n, MCHUNK);
    hipLaunchKernelGGL(head_write2_kernel, dim3((unsigned)nblk), dim3(CT), 0, st, mk, mc, n, partial, reinterpret_cast<K2*>(out_k2), out_c);
    return hipGetLastError();
}

}  // namespace kmx
