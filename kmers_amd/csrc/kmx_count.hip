// kmx_count.hip -- exact canonical k-mer counting (kmx_count_canonical, kmx_count_canonical2) and the union of two count tables
// (kmx_count_merge, kmx_count_merge2).  Every kernel is written once, templated on the words W of a key (Key<W>, kmx_count_common.h):
// W = 1 for k <= 31, W = 2 for k = 33..64.
//
// Input: the batch's canonical words and flags as kmx_canonical_windows(2) writes them (W u64 and one byte per window, in the
// context's work buffer).  A key has at most 2k significant bits, so the sort is an MSD radix partition by the key's OWN bits,
// 8 bits per level from bit 2k down, followed by a sort of each small partition in LDS:
//   level pass (over every partition still larger than LEAF keys, as tiles of TILE keys):
//     count    per tile: a 256-bin LDS histogram of the digit, and what the tile knows about "every key is equal" (Same<W>, below)
//     colscan  per (partition, digit): exclusive scan of the digit's per-tile counts (a thread per column above level 0; a block
//              per column at level 0 and for partitions of more than COL_SERIAL tiles)
//     segfinal per partition: exclusive scan of the 256 digit totals; then ONE of
//              - every key equal: the partition is one run, written at once, no scatter (heavy hitters, poly-A)
//              - the digit was the last one (no bits below it): every digit bucket is one run, written at once, no scatter
//              - else each child bucket goes to the next level (more than LEAF keys) or into a leaf group: consecutive
//                small siblings up to LEAF_SMALL keys in all are sorted together (they are a contiguous range); a child of
//                LEAF_SMALL + 1 .. LEAF keys is a group of its own
//     scatter  per tile: every key to its child's range (LDS atomics for the in-tile position: the order inside a child is
//              free, the leaf sorts whole keys)
//   leaf       per group: bitonic sort in LDS, run-length encoding, the distinct keys and their counts at the group's start
//   one host round trip per level (how many partitions and tiles the next level has, how many leaf groups this one left)
// The levels ping-pong between two arrays of one key per window (the canonical words' own array and a second one).  Every
// run's key is written to `keys` and its count to the other array at the same index (Key<W>::count: the low word of the slot),
// and a byte at that index is set in `keep`; the ranges of different partitions never overlap, so nothing is ordered across
// blocks but by kernel boundaries.  The table is then the kept entries in index order -- ascending, because partitions are laid
// out in digit order -- and is compacted by a block count, a scan, and a write (keep_count_kernel, scan_single_kernel and
// compact_write_kernel of kmx_count_common.h, which the filter shares; one more host round trip for the number of distinct keys).  No block waits for another: cross-block results travel through kernel boundaries only.
// What the width changes, beside the key itself:
//   - a digit is bits [hi_bit - 8, hi_bit) of the whole key and, with two words, may straddle them (2k mod 8 != 0): Key<W>::bits;
//   - how a partition learns that all its keys are equal: the per-width policy Same<W>;
//   - the level cap (8 W digits) and the tile records of Same<2> in the work area.
// Leaf capacities: a group of up to LEAF_SMALL = 512 keys takes 4 W KiB of keys (two words: 11 KiB of LDS a block: eight blocks,
// the CU's 32 waves); a child of 513..4096 keys takes 32 W KiB (two words: 74 KiB a block, two blocks per CU).  The large capacity
// stays at 4096 for two-word keys because the partition arrays -- 2 KiB of digit totals per partition -- are bounded by
// n / (LEAF + 1) partitions: at 2048 they alone would take another byte per window, and on random reads nearly every key reaches
// a leaf through the small groups.  Bitonic strides of 16 elements and more read and write consecutive elements per lane group
// (conflict-free); strides 1, 2, 4, 8 are two-way conflicts on the b128 lane groups, exactly what the 8-byte layout pays at the
// same strides -- a lo plane / hi plane layout has the same pattern at twice the instructions, so the element layout stays.
#include "kmx_count_common.h"

namespace kmx {

namespace {

constexpr u32 TILE = 16384;                   // keys per block in the partition passes
constexpr u32 LEAF = 4096;                    // keys a leaf block sorts in LDS (32 W KiB of keys)
constexpr u32 LEAF_SMALL = 512;               // leaf groups are gathered up to this size: a shorter bitonic network, more blocks per CU
constexpr u32 RCHUNK = CT * 16;               // reads per block in the window-offset passes

// A partition of a level:
//   start      first index of the partition (output coordinates; level 0: the window array)
//   n          keys (level 0: windows, valid or not)
//   tile_base  first tile of the partition in this level's tile space
//   mn, mx     one-word keys only: the least and the greatest key (Same<1>)
//   hi_bit     bits not yet partitioned: the digit is bits [hi_bit - w, hi_bit), w = min(8, hi_bit)
//   skip       segfinal wrote the partition's runs itself: no scatter
template <u32 W> struct Seg;
template <> struct Seg<1> {
    u64 start, n, tile_base;
    unsigned long long mn, mx;
    u32 hi_bit, skip;
};
template <> struct Seg<2> {
    u64 start, n, tile_base;
    u32 hi_bit, skip;
};

// ---------------------------------------------------------------- "every key of the partition is equal", per width
// Same<W> is what a thread of the count pass carries over its keys.  Each width provides:
//   Tile, TILE_BYTES   the record a tile leaves in the work area for segfinal (one word: none, 0 bytes)
//   Shared             the block's LDS for the fold
//   seg(...)           a fresh partition record (one word: with mn / mx at their neutral values)
//   init               before the first barrier of a kernel that folds
//   see                per key: what the thread remembers
//   fold, publish      per tile: the block's fold (its barriers also close the histogram), then what thread 0 leaves for segfinal
//   resolve            in segfinal: "the partition holds one key" and a key of the partition (its bits above the digit are every key's)
// One word: the 64-bit min and max, one global atomicMin / atomicMax per tile into the partition's Seg; one key <=> mn == mx.
// Two words have no 64-bit min / max to lean on: a thread compares its keys with the first one it met, a tile leaves {a key of its
// own, has keys, keys differ} in a record per tile, and the partition's finalise block folds its tiles' records the same way.  No
// atomic on global memory, no order between blocks; an all-A batch still costs the window pass and one count pass.
template <u32 W> struct Same;
template <> struct Same<1> {
    struct Tile {};   // (no record per tile: TILE_BYTES of the work area)
    static constexpr size_t TILE_BYTES = 0;
    struct Shared {
        unsigned long long red[2][CT / 64];
    };
    unsigned long long mn = ~0ull, mx = 0ull;
    __device__ __forceinline__ static Seg<1> seg(u64 start, u64 n, u64 tile_base, u32 hi_bit) {
        return Seg<1>{start, n, tile_base, ~0ull, 0ull, hi_bit, 0u};
    }
    __device__ __forceinline__ static void init(Shared*) {}
    __device__ __forceinline__ void see(const Key<1>& key) {
        mn = key.lo < mn ? key.lo : mn;
        mx = key.lo > mx ? key.lo : mx;
    }
    __device__ __forceinline__ void fold(Shared* sm) {
        for (u32 o = 32; o > 0; o >>= 1) {
            const unsigned long long a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
        if ((threadIdx.x & 63u) == 0) {
            sm->red[0][threadIdx.x >> 6] = mn;
            sm->red[1][threadIdx.x >> 6] = mx;
        }
        __syncthreads();
    }
    __device__ __forceinline__ void publish(const Shared* sm, Seg<1>* seg, Tile*) {
        if (threadIdx.x == 0) {
            for (u32 j = 1; j < CT / 64; ++j) {
                mn = sm->red[0][j] < mn ? sm->red[0][j] : mn;
                mx = sm->red[1][j] > mx ? sm->red[1][j] : mx;
            }
            if (mn != ~0ull) atomicMin(&seg->mn, mn);
            if (mx != 0ull) atomicMax(&seg->mx, mx);
        }
    }
    __device__ __forceinline__ static bool resolve(Shared*, const Seg<1>& s, const Tile*, Key<1>* ref) {
        *ref = Key<1>{s.mn};
        return s.mn == s.mx;
    }
};
template <> struct Same<2> {
    // what a tile's count pass says about its keys (a record per tile of the level)
    struct Tile {
        Key<2> ref;     // one of the tile's keys (if it has any)
        u32 state;      // HAS: the tile holds a key; DIFF: not all of them equal `ref`
        u32 pad[3];
    };
    static constexpr size_t TILE_BYTES = sizeof(Tile);
    static constexpr u32 HAS = 1u, DIFF = 2u;
    // the block's fold: the reference is the key of the lowest thread that has one, so the result does not depend on timing
    struct Shared {
        Key<2> ref;
        u32 first, state;
    };
    // (in this order: the count kernels keep the instruction order they were built with; the compiler follows the members' order)
    Key<2> f{0u, 0u};   // the first key the thread met
    bool diff = false;
    bool has = false;
    __device__ __forceinline__ static Seg<2> seg(u64 start, u64 n, u64 tile_base, u32 hi_bit) { return Seg<2>{start, n, tile_base, hi_bit, 0u}; }
    // (a barrier lies between init and fold)
    __device__ __forceinline__ static void init(Shared* sm) {
        if (threadIdx.x == 0) {
            sm->first = CT;
            sm->state = 0u;
        }
    }
    __device__ __forceinline__ void see(const Key<2>& key) {
        if (!has) {
            f = key;
            has = true;
        } else {
            diff |= key.differs(f);
        }
    }
    // on return sm->state and sm->ref hold the block's
    __device__ __forceinline__ void fold(Shared* sm) {
        if (has) atomicMin(&sm->first, threadIdx.x);
        __syncthreads();
        if (threadIdx.x == sm->first) {
            sm->ref = f;
            sm->state = HAS;
        }
        __syncthreads();
        if (has && (diff || f.differs(sm->ref))) atomicOr(&sm->state, DIFF);
        __syncthreads();
    }
    __device__ __forceinline__ void publish(const Shared* sm, Seg<2>*, Tile* tkeys) {
        if (threadIdx.x == 0) tkeys[blockIdx.x] = Tile{sm->ref, sm->state, {0u, 0u, 0u}};
    }
    // the tiles' records, folded as a tile folds its keys
    __device__ __forceinline__ static bool resolve(Shared* sm, const Seg<2>& s, const Tile* tkeys, Key<2>* ref) {
        const u64 nt = ceil_div(s.n, TILE);
        Same<2> same;
        for (u64 t = threadIdx.x; t < nt; t += CT) {
            const Tile tk = tkeys[s.tile_base + t];
            if (!(tk.state & HAS)) continue;
            same.diff |= (tk.state & DIFF) != 0;
            same.see(tk.ref);
        }
        same.fold(sm);
        *ref = sm->ref;
        return !(sm->state & DIFF);
    }
};

// ---------------------------------------------------------------- window offsets of ragged reads
// (a read of 2^31 bases or more owns no window: the scans skip it and report it, kmx.h "Limits")
__device__ __forceinline__ u64 read_windows(const u64* offsets, u64 r, u32 k) {
    const u64 len = offsets[r + 1u] - offsets[r];
    return len >= k && len <= 0x7FFFFFFFull ? len - k + 1u : 0u;
}

__global__ void __launch_bounds__(CT) win_count_kernel(const u64* __restrict__ offsets, u64 n_reads, u32 k, u64* __restrict__ partial) {
    __shared__ u64 sh[CT];
    const u64 r0 = (u64)blockIdx.x * RCHUNK + (u64)threadIdx.x * 16u;
    u64 s = 0;
    for (u32 j = 0; j < 16; ++j)
        if (r0 + j < n_reads) s += read_windows(offsets, r0 + j, k);
    u64 tot;
    (void)block_exscan(s, sh, &tot);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(CT) win_fill_kernel(const u64* __restrict__ offsets, u64 n_reads, u32 k, const u64* __restrict__ partial,
                                                      u64* __restrict__ wo) {
    __shared__ u64 sh[CT];
    const u64 r0 = (u64)blockIdx.x * RCHUNK + (u64)threadIdx.x * 16u;
    u64 w[16], s = 0;
    for (u32 j = 0; j < 16; ++j) {
        w[j] = r0 + j < n_reads ? read_windows(offsets, r0 + j, k) : 0u;
        s += w[j];
    }
    u64 tot;
    u64 run = partial[blockIdx.x] + block_exscan(s, sh, &tot);
    for (u32 j = 0; j < 16; ++j) {
        if (r0 + j < n_reads) wo[r0 + j] = run;
        run += w[j];
    }
    if (blockIdx.x == gridDim.x - 1u && threadIdx.x == CT - 1u) wo[n_reads] = run;
}

// ---------------------------------------------------------------- one level of the partition
template <u32 W>
__device__ __forceinline__ void tile_range(const Seg<W>& s, u64 t_local, u64* lo, u64* hi) {
    *lo = s.start + t_local * TILE;
    const u64 e = *lo + TILE, end = s.start + s.n;
    *hi = e < end ? e : end;
}

// L0: the input is the window array (canon + flags, invalid windows dropped); above: the keys of the partitions
template <u32 W, bool L0>
__global__ void __launch_bounds__(CT) count_kernel(Seg<W>* __restrict__ segs, const u32* __restrict__ tile_seg, const u64* __restrict__ in,
                                                   const uint8_t* __restrict__ flags, u64* __restrict__ hist,
                                                   typename Same<W>::Tile* __restrict__ tkeys) {
    __shared__ u32 h[RADIX];
    __shared__ typename Same<W>::Shared sm;
    const u32 si = L0 ? 0u : tile_seg[blockIdx.x];
    const Seg<W> s = segs[si];
    const u64 t_local = blockIdx.x - s.tile_base, nt = ceil_div(s.n, TILE);
    const u32 w = digit_width(s.hi_bit), sh = s.hi_bit - w, mask = (1u << w) - 1u;
    h[threadIdx.x] = 0;
    Same<W>::init(&sm);
    __syncthreads();
    u64 lo, hi;
    tile_range(s, t_local, &lo, &hi);
    Same<W> same;
    for (u64 i = lo + threadIdx.x; i < hi; i += CT) {
        if (L0 && !(flags[i] & KMX_WIN_VALID)) continue;
        const Key<W> key = Key<W>::load(in, i);
        atomicAdd(&h[key.bits(sh) & mask], 1u);
        same.see(key);
    }
    same.fold(&sm);   // (its barriers also close the histogram)
    hist[s.tile_base * RADIX + (u64)threadIdx.x * nt + t_local] = h[threadIdx.x];
    same.publish(&sm, &segs[si], tkeys);
}

// a block per (partition, digit): the digit's per-tile counts -> exclusive prefix; the digit's total -> coltot.  Level 0: its one
// partition; above: the partitions of more than COL_SERIAL tiles, listed in `big` (a heavy hitter's partition holds most of the batch)
template <u32 W>
__global__ void __launch_bounds__(CT) colscan_kernel(const Seg<W>* __restrict__ segs, const u32* __restrict__ big, u64* __restrict__ hist,
                                                     u64* __restrict__ coltot) {
    __shared__ u64 sh[CT];
    const u32 si = big ? big[blockIdx.x / RADIX] : blockIdx.x / RADIX, b = blockIdx.x % RADIX;
    const Seg<W> s = segs[si];
    const u64 nt = ceil_div(s.n, TILE);
    u64 tot;
    block_scan_array(hist + s.tile_base * RADIX + (u64)b * nt, nt, sh, &tot);
    if (threadIdx.x == 0) coltot[(u64)si * RADIX + b] = tot;
}

// levels above 0: a block per partition of at most COL_SERIAL tiles, a thread per digit walking its column (longer ones: above)
template <u32 W>
__global__ void __launch_bounds__(CT) colscan_seg_kernel(const Seg<W>* __restrict__ segs, u64* __restrict__ hist, u64* __restrict__ coltot) {
    const Seg<W> s = segs[blockIdx.x];
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

// a block per partition: the digit totals -> the children's bases (in coltot, relative to the partition's start); "one key" from
// Same<W>; the partition's runs if it needs no scatter; else its children to the next level and the leaf groups
template <u32 W>
__global__ void __launch_bounds__(CT) segfinal_kernel(Seg<W>* __restrict__ segs, u64* __restrict__ coltot, Seg<W>* __restrict__ next, u64 max_next,
                                                      u32* __restrict__ big, u64 max_big,
                                                      Leaf* __restrict__ leaves, u64 max_leaf, Leaf* __restrict__ small, u64 max_small,
                                                      Counters* __restrict__ cnt, u32 dst_is_keys,
                                                      u64* __restrict__ keys, u64* __restrict__ other, uint8_t* __restrict__ keep, u32 level0,
                                                      const typename Same<W>::Tile* __restrict__ tkeys) {
    __shared__ u64 sh[CT];
    __shared__ typename Same<W>::Shared sm;
    const u32 si = blockIdx.x;
    const Seg<W> s = segs[si];
    Same<W>::init(&sm);
    const u64 v = coltot[(u64)si * RADIX + threadIdx.x];
    u64 total;
    const u64 base = block_exscan(v, sh, &total);
    coltot[(u64)si * RADIX + threadIdx.x] = base;
    if (level0 && threadIdx.x == 0) cnt->n_valid = total;
    if (total == 0) {
        if (threadIdx.x == 0) segs[si].skip = 1u;
        return;
    }
    Key<W> ref;
    const bool one = Same<W>::resolve(&sm, s, tkeys, &ref);
    const u32 w = digit_width(s.hi_bit), shift = s.hi_bit - w;
    if (one) {            // one key: one run
        if (threadIdx.x == 0) {
            Key<W>::store(keys, s.start, ref);
            Key<W>::store(other, s.start, Key<W>::count(total));
            keep[s.start] = 1u;
            segs[si].skip = 1u;
        }
        return;
    }
    if (shift == 0) {     // the last digit: every bucket is one key (the bits above it are the partition's own)
        if (v != 0) {
            const u64 at = s.start + base;
            Key<W>::store(keys, at, ref.with_low(w, threadIdx.x));
            Key<W>::store(other, at, Key<W>::count(v));
            keep[at] = 1u;
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
    // then reserves the slots -- an atomic per record on one counter serialised ~65k partitions at 1.2e9 keys), the second writes
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
                    next[i_nx] = Same<W>::seg(sb, nb, i_tile, shift);
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

template <u32 W, bool L0>
__global__ void __launch_bounds__(CT) scatter_kernel(const Seg<W>* __restrict__ segs, const u32* __restrict__ tile_seg, const u64* __restrict__ in,
                                                     const uint8_t* __restrict__ flags, const u64* __restrict__ hist,
                                                     const u64* __restrict__ coltot, u64* __restrict__ out) {
    __shared__ u64 pos[RADIX];
    __shared__ u32 fill[RADIX];
    const u32 si = L0 ? 0u : tile_seg[blockIdx.x];
    const Seg<W> s = segs[si];
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
        const Key<W> key = Key<W>::load(in, i);
        const u32 d = key.bits(sh) & mask;
        Key<W>::store(out, pos[d] + atomicAdd(&fill[d], 1u), key);
    }
}

// level 0: one partition, the whole window array
template <u32 W>
__global__ void seg_init_kernel(Seg<W>* __restrict__ segs, u64 n_win, u32 hi_bit) { segs[0] = Same<W>::seg(0u, n_win, 0u, hi_bit); }

// the tiles of the next level's partitions -> their partition
template <u32 W>
__global__ void __launch_bounds__(CT) tilemap_kernel(const Seg<W>* __restrict__ segs, u32* __restrict__ tile_seg) {
    const Seg<W> s = segs[blockIdx.x];
    const u64 nt = ceil_div(s.n, TILE);
    for (u64 j = threadIdx.x; j < nt; j += CT) tile_seg[s.tile_base + j] = blockIdx.x;
}

// a block per leaf group of at most CAP keys: bitonic sort in LDS (a key is one element), run-length encoding
template <u32 W, u32 CAP>
__global__ void __launch_bounds__(CT) leaf_kernel(const Leaf* __restrict__ leaves, u64* __restrict__ keys, u64* __restrict__ other,
                                                  uint8_t* __restrict__ keep) {
    __shared__ Key<W> a[CAP];
    __shared__ uint16_t head_at[CAP];
    __shared__ u64 sh[CT];
    const Leaf L = leaves[blockIdx.x];
    const u32 n = (u32)L.n;
    const u64* src = L.in_keys ? keys : other;
    u32 P = 2;
    while (P < n) P <<= 1;
    for (u32 i = threadIdx.x; i < P; i += CT) a[i] = i < n ? Key<W>::load(src, L.start + i) : Key<W>::sentinel();
    for (u32 size = 2; size <= P; size <<= 1) {
        for (u32 stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (u32 t = threadIdx.x; t < (P >> 1); t += CT) {
                const u32 i = 2u * t - (t & (stride - 1u)), j = i + stride;
                const bool up = (i & size) == 0;
                const Key<W> x = a[i], y = a[j];
                if (x.greater(y) == up) {
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
        if (i < n && (i == 0 || a[i].differs(a[i - 1u]))) ++heads;
    }
    u64 nd;
    u32 r = (u32)block_exscan(heads, sh, &nd);
    for (u32 j = 0; j < PER; ++j) {
        const u32 i = i0 + j;
        if (i < n && (i == 0 || a[i].differs(a[i - 1u]))) head_at[r++] = (uint16_t)i;
    }
    __syncthreads();
    for (u32 q = threadIdx.x; q < (u32)nd; q += CT) {
        const u32 p = head_at[q], e = q + 1u < (u32)nd ? (u32)head_at[q + 1u] : n;
        Key<W>::store(keys, L.start + q, a[p]);
        Key<W>::store(other, L.start + q, Key<W>::count(e - p));
        keep[L.start + q] = 1u;
    }
}

// ---------------------------------------------------------------- merge of two tables
// merge path: thread t writes outputs [8 t, 8 t + 8); on equal keys the item of `a` goes first
// ka[i] <= kb[j].  Spelled per width, as each kernel was built: the compiler keeps the order of the loads and of the operands it
// is given, and one spelling for both would change the instructions of one of them.
template <u32 W>
__device__ __forceinline__ bool a_first(const u64* __restrict__ ka, u64 i, const u64* __restrict__ kb, u64 j) {
    if constexpr (W == 1) return !Key<W>::load(ka, i).greater(Key<W>::load(kb, j));
    else return !Key<W>::load(kb, j).less(Key<W>::load(ka, i));
}

template <u32 W>
__global__ void __launch_bounds__(CT) merge_kernel(const u64* __restrict__ ka, const u64* __restrict__ ca, u64 na, const u64* __restrict__ kb,
                                                   const u64* __restrict__ cb, u64 nb, u64* __restrict__ mk, u64* __restrict__ mc) {
    const u64 n = na + nb, d = ((u64)blockIdx.x * CT + threadIdx.x) * MERGE_IPT;
    if (d >= n) return;
    u64 lo = d > nb ? d - nb : 0u, hi = d < na ? d : na;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (a_first<W>(ka, mid, kb, d - 1u - mid)) lo = mid + 1u;
        else hi = mid;
    }
    u64 i = lo, j = d - lo;
    // The walk is spelled per width, as each was built and measured: one word compares the heads where they lie and reads the
    // winner again for the store; two words load both heads once (two dwordx4) and store from registers.  The two compile to
    // different code for either width, so making them one belongs in a change that is measured as such.
    for (u32 q = 0; q < MERGE_IPT && d + q < n; ++q) {
        if constexpr (W == 1) {
            if (j >= nb || (i < na && a_first<W>(ka, i, kb, j))) {
                Key<W>::store(mk, d + q, Key<W>::load(ka, i));
                mc[d + q] = ca[i];
                ++i;
            } else {
                Key<W>::store(mk, d + q, Key<W>::load(kb, j));
                mc[d + q] = cb[j];
                ++j;
            }
        } else {
            bool take_a = j >= nb;
            Key<W> x = Key<W>::count(0u), y = Key<W>::count(0u);   // (all zero)
            if (i < na) x = Key<W>::load(ka, i);
            if (j < nb) y = Key<W>::load(kb, j);
            if (!take_a && i < na) take_a = !y.less(x);
            if (take_a) {
                Key<W>::store(mk, d + q, x);
                mc[d + q] = ca[i];
                ++i;
            } else {
                Key<W>::store(mk, d + q, y);
                mc[d + q] = cb[j];
                ++j;
            }
        }
    }
}

template <u32 W>
__device__ __forceinline__ bool is_head(const u64* mk, u64 i) { return i == 0 || Key<W>::load(mk, i).differs(Key<W>::load(mk, i - 1u)); }

template <u32 W>
__global__ void __launch_bounds__(CT) head_count_kernel(const u64* __restrict__ mk, u64 n, u64* __restrict__ partial) {
    __shared__ u64 sh[CT];
    const u64 i0 = (u64)blockIdx.x * MCHUNK + (u64)threadIdx.x * 16u;
    u64 c = 0;
    for (u32 j = 0; j < 16; ++j)
        if (i0 + j < n && is_head<W>(mk, i0 + j)) ++c;
    u64 tot;
    (void)block_exscan(c, sh, &tot);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

template <u32 W>
__global__ void __launch_bounds__(CT) head_write_kernel(const u64* __restrict__ mk, const u64* __restrict__ mc, u64 n, const u64* __restrict__ partial,
                                                        u64* __restrict__ out_k, u64* __restrict__ out_c) {
    __shared__ u64 sh[CT];
    const u64 i0 = (u64)blockIdx.x * MCHUNK + (u64)threadIdx.x * 16u;
    u64 c = 0;
    for (u32 j = 0; j < 16; ++j)
        if (i0 + j < n && is_head<W>(mk, i0 + j)) ++c;
    u64 tot;
    u64 o = partial[blockIdx.x] + block_exscan(c, sh, &tot);
    for (u32 j = 0; j < 16; ++j) {
        const u64 i = i0 + j;
        if (i < n && is_head<W>(mk, i)) {
            // (each table holds a key once: an equal neighbour is the other table's entry)
            Key<W>::copy(out_k, o, mk, i);
            out_c[o] = mc[i] + (i + 1u < n && !Key<W>::load(mk, i + 1u).differs(Key<W>::load(mk, i)) ? mc[i + 1u] : 0u);
            ++o;
        }
    }
}

// bounds of one level's arrays for n keys
u64 max_segs(u64 n) { return n / (LEAF + 1u) + 2u; }
u64 max_tiles(u64 n) { return ceil_div(n, TILE) + max_segs(n) + 1u; }
// Leaf groups of one level: their ranges are disjoint.  A large group holds more than LEAF_SMALL keys, so there are at most
// n / (LEAF_SMALL + 1) of them.  Two small groups of one partition that follow each other either hold more than LEAF_SMALL keys
// together or have a larger child (a large group or a next-level partition, at most n / (LEAF_SMALL + 1) in all) between them,
// so a partition has at most 1 + 2 keys / (LEAF_SMALL + 1) + its larger children small groups.
u64 max_big(u64 n) { return ceil_div(n, (u64)COL_SERIAL * TILE) + 2u; }   // partitions of more than COL_SERIAL tiles
u64 max_leaves(u64 n) { return ceil_div(n, LEAF_SMALL + 1u) + 64u; }
u64 max_small_leaves(u64 n) { return 3u * ceil_div(n, LEAF_SMALL + 1u) + max_segs(n) + 64u; }

// ---------------------------------------------------------------- host side
// The work area of one count, after the canon / flags arrays: keys (8 W B per window), keep (1 B per window), then the level
// arrays (two words: ~1.35 B per window: 2 KiB of tile histograms per tile and of digit bases per partition, the tile records,
// the leaf lists).  `n` = the windows the area is sized for.
template <u32 W>
struct CountArea {
    u64* keys;
    uint8_t* keep;
    u64* hist;
    u64* coltot;
    u32* tile_seg;
    u32* big;
    typename Same<W>::Tile* tkeys;   // (two-word keys only)
    Seg<W>* segs[2];
    Leaf* leaves;
    Leaf* small;
    u64* partial;
    Counters* cnt;
    size_t keep_bytes;
};

template <u32 W>
size_t area_layout(u64 n, CountArea<W>* out, void* base) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += align256(bytes);
        return base ? static_cast<char*>(base) + at : nullptr;
    };
    CountArea<W> a{};
    a.keys = reinterpret_cast<u64*>(take(8u * W * n));
    a.keep_bytes = ceil_div(n, CHUNK) * CHUNK;
    a.keep = reinterpret_cast<uint8_t*>(take(a.keep_bytes));
    a.hist = reinterpret_cast<u64*>(take(8u * RADIX * max_tiles(n)));
    a.coltot = reinterpret_cast<u64*>(take(8u * RADIX * max_segs(n)));
    a.tile_seg = reinterpret_cast<u32*>(take(4u * max_tiles(n)));
    a.big = reinterpret_cast<u32*>(take(4u * max_big(n)));
    a.tkeys = reinterpret_cast<typename Same<W>::Tile*>(take(Same<W>::TILE_BYTES * max_tiles(n)));
    a.segs[0] = reinterpret_cast<Seg<W>*>(take(sizeof(Seg<W>) * max_segs(n)));
    a.segs[1] = reinterpret_cast<Seg<W>*>(take(sizeof(Seg<W>) * max_segs(n)));
    a.leaves = reinterpret_cast<Leaf*>(take(sizeof(Leaf) * max_leaves(n)));
    a.small = reinterpret_cast<Leaf*>(take(sizeof(Leaf) * max_small_leaves(n)));
    a.partial = reinterpret_cast<u64*>(take(8u * (ceil_div(n, CHUNK) + 2u)));
    a.cnt = reinterpret_cast<Counters*>(take(sizeof(Counters)));
    if (out) *out = a;
    return off;
}

template <u32 W>
hipError_t count_sort(u64* canon, const uint8_t* flags, u64 n_win, u32 k, void* area, unsigned long long* h_pinned, u64* h_valid, u64* h_distinct,
                      bool* bad, hipStream_t st) {
    CountArea<W> a;
    area_layout<W>(n_win, &a, area);
    *bad = false;
    hipError_t e;
    if ((e = hipMemsetAsync(a.keep, 0, a.keep_bytes, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(seg_init_kernel<W>, dim3(1), dim3(1), 0, st, a.segs[0], n_win, 2u * k);
    const u64 ms = max_segs(n_win), ml = max_leaves(n_win), mls = max_small_leaves(n_win), mt = max_tiles(n_win), mb = max_big(n_win);
    u64 n_seg = 1, n_tiles = ceil_div(n_win, TILE), n_big = 0;
    *h_valid = 0;
    for (u32 level = 0; n_seg != 0; ++level) {
        if (level > 8u * W) {   // (2k <= 64 W bits: at most 8 W digits)
            *bad = true;
            return hipSuccess;
        }
        const bool l0 = level == 0;
        Seg<W>* cur = a.segs[level & 1u];
        Seg<W>* nxt = a.segs[(level & 1u) ^ 1u];
        // level 0 reads the windows (canon) and writes `keys`; then the levels alternate
        const bool src_is_keys = (level & 1u) == 1u;
        u64* src = src_is_keys ? a.keys : canon;
        u64* dst = src_is_keys ? canon : a.keys;
        if ((e = hipMemsetAsync(a.cnt, 0, LEVEL_COUNTERS, st)) != hipSuccess) return e;
        if (l0) hipLaunchKernelGGL((count_kernel<W, true>), dim3((unsigned)n_tiles), dim3(CT), 0, st, cur, a.tile_seg, src, flags, a.hist, a.tkeys);
        else hipLaunchKernelGGL((count_kernel<W, false>), dim3((unsigned)n_tiles), dim3(CT), 0, st, cur, a.tile_seg, src, flags, a.hist, a.tkeys);
        if (l0) {
            hipLaunchKernelGGL(colscan_kernel<W>, dim3(RADIX), dim3(CT), 0, st, cur, (const u32*)nullptr, a.hist, a.coltot);
        } else {
            hipLaunchKernelGGL(colscan_seg_kernel<W>, dim3((unsigned)n_seg), dim3(CT), 0, st, cur, a.hist, a.coltot);
            if (n_big) hipLaunchKernelGGL(colscan_kernel<W>, dim3((unsigned)(n_big * RADIX)), dim3(CT), 0, st, cur, (const u32*)a.big, a.hist, a.coltot);
        }
        hipLaunchKernelGGL(segfinal_kernel<W>, dim3((unsigned)n_seg), dim3(CT), 0, st, cur, a.coltot, nxt, ms, a.big, mb, a.leaves, ml, a.small, mls, a.cnt,
                           src_is_keys ? 0u : 1u, a.keys, canon, a.keep, l0 ? 1u : 0u, a.tkeys);
        if (l0) hipLaunchKernelGGL((scatter_kernel<W, true>), dim3((unsigned)n_tiles), dim3(CT), 0, st, cur, a.tile_seg, src, flags, a.hist, a.coltot, dst);
        else hipLaunchKernelGGL((scatter_kernel<W, false>), dim3((unsigned)n_tiles), dim3(CT), 0, st, cur, a.tile_seg, src, flags, a.hist, a.coltot, dst);
        u64 c[LEVEL_COUNTERS / 8u];   // (in the order of Counters)
        if ((e = read_back(h_pinned, a.cnt, LEVEL_COUNTERS / 8u, c, st)) != hipSuccess) return e;
        if (l0) *h_valid = c[0];
        const u64 n_next = c[1], n_next_tiles = c[2], n_leaf = c[3], n_small = c[5], n_next_big = c[6];
        if (c[4] != 0 || n_next > ms || n_leaf > ml || n_small > mls || n_next_tiles > mt || n_next_big > mb) {
            *bad = true;
            return hipSuccess;
        }
        if (n_leaf) hipLaunchKernelGGL((leaf_kernel<W, LEAF>), dim3((unsigned)n_leaf), dim3(CT), 0, st, a.leaves, a.keys, canon, a.keep);
        if (n_small) hipLaunchKernelGGL((leaf_kernel<W, LEAF_SMALL>), dim3((unsigned)n_small), dim3(CT), 0, st, a.small, a.keys, canon, a.keep);
        if (n_next) hipLaunchKernelGGL(tilemap_kernel<W>, dim3((unsigned)n_next), dim3(CT), 0, st, nxt, a.tile_seg);
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
    return read_back(h_pinned, &a.cnt->n_distinct, 1u, h_distinct, st);
}

template <u32 W>
hipError_t count_emit(const u64* canon, u64 n_win, u64 n_valid, void* area, u64* out_k, u64* out_c, hipStream_t st) {
    CountArea<W> a;
    area_layout<W>(n_win, &a, area);
    const u64 nb = ceil_div(n_valid, CHUNK);
    if (nb) hipLaunchKernelGGL((compact_write_kernel<W, W>), dim3((unsigned)nb), dim3(CT), 0, st, a.keep, a.partial, a.keys, canon, out_k, out_c);
    return hipGetLastError();
}

// the merge's work area: merged keys (8 W B per input entry), their counts (8 B), the blocks' head counts
struct MergeArea {
    u64 *mk, *mc, *partial;
};
MergeArea merge_layout(u32 words, u64 n, const void* area) {
    char* base = static_cast<char*>(const_cast<void*>(area));
    const size_t mc_at = align256(8u * words * n), partial_at = mc_at + align256(8u * n);
    return MergeArea{reinterpret_cast<u64*>(base), reinterpret_cast<u64*>(base + mc_at), reinterpret_cast<u64*>(base + partial_at)};
}

}  // namespace

// (`words` u64 per key, 1 or 2, as in the query and set-operation launchers; two-word key arrays are 16-byte aligned, low word first)
size_t count_area_bytes(u32 words, u64 n) { return words == 1u ? area_layout<1>(n, nullptr, nullptr) : area_layout<2>(n, nullptr, nullptr); }

size_t win_offsets_bytes(u64 n_reads) { return align256(8u * (n_reads + 1u)) + align256(8u * (ceil_div(n_reads, RCHUNK) + 2u)); }

// ragged reads: wo[r] = exclusive prefix of max(len_r - k + 1, 0), wo[n_reads] = the total, which comes back to *h_total
hipError_t launch_count_win_offsets(const u64* offsets, u64 n_reads, u32 k, void* area, u64** wo_out, unsigned long long* h_pinned,
                                    u64* h_total, hipStream_t st) {
    u64* wo = static_cast<u64*>(area);
    u64* partial = reinterpret_cast<u64*>(static_cast<char*>(area) + align256(8u * (n_reads + 1u)));
    const u64 nb = ceil_div(n_reads, RCHUNK);
    hipLaunchKernelGGL(win_count_kernel, dim3((unsigned)nb), dim3(CT), 0, st, offsets, n_reads, k, partial);
    hipLaunchKernelGGL(scan_single_kernel, dim3(1), dim3(CT), 0, st, partial, nb, partial + nb);
    hipLaunchKernelGGL(win_fill_kernel, dim3((unsigned)nb), dim3(CT), 0, st, offsets, n_reads, k, partial, wo);
    *wo_out = wo;
    return read_back(h_pinned, wo + n_reads, 1u, h_total, st);
}

// Sort and tally the n_win windows (canon / flags) of a batch of k-mers; the table is left in `area` (keys in a.keys, counts
// in the low words of canon's slots, marked in a.keep) and its size comes back in *h_distinct.  Synchronous: one host round trip
// per level and one for the number of distinct keys.  *bad: the level arrays overflowed their bounds (a bug, never expected).
hipError_t launch_count_sort(u32 words, u64* canon, const uint8_t* flags, u64 n_win, u32 k, void* area, unsigned long long* h_pinned, u64* h_valid,
                             u64* h_distinct, bool* bad, hipStream_t st) {
    return words == 1u ? count_sort<1>(canon, flags, n_win, k, area, h_pinned, h_valid, h_distinct, bad, st)
                       : count_sort<2>(canon, flags, n_win, k, area, h_pinned, h_valid, h_distinct, bad, st);
}

// the table launch_count_sort left in `area` -> out_k / out_c (n_distinct entries)
hipError_t launch_count_emit(u32 words, const u64* canon, u64 n_win, u64 n_valid, void* area, u64* out_k, u64* out_c, hipStream_t st) {
    return words == 1u ? count_emit<1>(canon, n_win, n_valid, area, out_k, out_c, st) : count_emit<2>(canon, n_win, n_valid, area, out_k, out_c, st);
}

size_t count_merge_bytes(u32 words, u64 n) { return align256(8u * words * n) + align256(8u * n) + align256(8u * (ceil_div(n, MCHUNK) + 2u)); }

// merge of two tables into `area` and the number of distinct keys of the union (synchronous: one host round trip)
hipError_t launch_count_merge(u32 words, const u64* ka, const u64* ca, u64 na, const u64* kb, const u64* cb, u64 nb, void* area,
                              unsigned long long* h_pinned, u64* h_out, hipStream_t st) {
    const u64 n = na + nb, nblk = ceil_div(n, MCHUNK);
    const MergeArea a = merge_layout(words, n, area);
    const dim3 gm((unsigned)ceil_div(n, (u64)CT * MERGE_IPT)), gh((unsigned)nblk), b(CT);
    with_width(words, [&](auto w) {
        hipLaunchKernelGGL(merge_kernel<decltype(w)::value>, gm, b, 0, st, ka, ca, na, kb, cb, nb, a.mk, a.mc);
        hipLaunchKernelGGL(head_count_kernel<decltype(w)::value>, gh, b, 0, st, (const u64*)a.mk, n, a.partial);
    });
    hipLaunchKernelGGL(scan_single_kernel, dim3(1), dim3(CT), 0, st, a.partial, nblk, a.partial + nblk);
    return read_back(h_pinned, a.partial + nblk, 1u, h_out, st);
}

hipError_t launch_count_merge_emit(u32 words, u64 n, const void* area, u64* out_k, u64* out_c, hipStream_t st) {
    const MergeArea a = merge_layout(words, n, area);
    const dim3 g((unsigned)ceil_div(n, MCHUNK)), b(CT);
    if (words == 1u) hipLaunchKernelGGL(head_write_kernel<1>, g, b, 0, st, (const u64*)a.mk, (const u64*)a.mc, n, (const u64*)a.partial, out_k, out_c);
    else hipLaunchKernelGGL(head_write_kernel<2>, g, b, 0, st, (const u64*)a.mk, (const u64*)a.mc, n, (const u64*)a.partial, out_k, out_c);
    return hipGetLastError();
}

}  // namespace kmx
