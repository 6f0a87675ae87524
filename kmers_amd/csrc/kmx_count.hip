// kmx_count.hip -- exact canonical k-mer counting (kmx_count_canonical) and the union of two count tables (kmx_count_merge).
//
// Input: the batch's canonical words and flags as kmx_canonical_windows writes them (one u64 and one byte per window, in the
// context's work buffer).  A key has at most 2k significant bits, so the sort is an MSD radix partition by the key's OWN bits,
// 8 bits per level from bit 2k down, followed by a sort of each small partition in LDS:
//   level pass (over every partition still larger than LEAF keys, as tiles of TILE keys):
//     count    per tile: a 256-bin LDS histogram of the digit, the min and the max key of the partition (global atomics, one per tile)
//     colscan  per (partition, digit): exclusive scan of the digit's per-tile counts (a thread per column above level 0; a block
//              per column at level 0 and for partitions of more than COL_SERIAL tiles)
//     segfinal per partition: exclusive scan of the 256 digit totals; then ONE of
//              - every key equal (min == max): the partition is one run, written at once, no scatter (heavy hitters, poly-A)
//              - the digit was the last one (no bits below it): every digit bucket is one run, written at once, no scatter
//              - else each child bucket goes to the next level (more than LEAF keys) or into a leaf group: consecutive
//                small siblings up to LEAF_SMALL keys in all are sorted together (they are a contiguous range); a child of
//                LEAF_SMALL + 1 .. LEAF keys is a group of its own
//     scatter  per tile: every key to its child's range (LDS atomics for the in-tile position: the order inside a child is
//              free, the leaf sorts whole keys)
//   leaf       per group: bitonic sort in LDS, run-length encoding, the distinct keys and their counts at the group's start
//   one host round trip per level (how many partitions and tiles the next level has, how many leaf groups this one left)
// The levels ping-pong between two arrays of one u64 per window (the canonical words' own array and a second one).  Every
// run's key is written to `keys` and its count to the other array at the same index, and a byte at that index is set in
// `keep`; the ranges of different partitions never overlap, so nothing is ordered across blocks but by kernel boundaries.
// The table is then the kept entries in index order -- ascending, because partitions are laid out in digit order -- and
// is compacted by a block count, a scan, and a write (one more host round trip for the number of distinct keys).
// No block waits for another: cross-block results travel through kernel boundaries only.
// (what does not depend on the width of a key -- block scans, the Leaf / Counters records, the count of the marked bytes -- is in
// kmx_count_common.h, shared with the two-word counter of kmx_count2.hip)
#include "kmx_count_common.h"

namespace kmx {

namespace {

constexpr u32 TILE = 16384;                   // keys per block in the partition passes
constexpr u32 LEAF = 4096;                    // keys a leaf block sorts in LDS (32 KiB of keys)
constexpr u32 LEAF_SMALL = 512;               // leaf groups are gathered up to this size: a shorter bitonic network, more blocks per CU
constexpr u32 RCHUNK = CT * 16;               // reads per block in the window-offset passes

struct Seg {
    u64 start;      // first index of the partition (output coordinates; level 0: the window array)
    u64 n;          // keys (level 0: windows, valid or not)
    u64 tile_base;  // first tile of the partition in this level's tile space
    unsigned long long mn, mx;
    u32 hi_bit;     // bits not yet partitioned: the digit is bits [hi_bit - w, hi_bit), w = min(8, hi_bit)
    u32 skip;       // segfinal wrote the partition's runs itself: no scatter
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
__device__ __forceinline__ void tile_range(const Seg& s, u64 t_local, u64* lo, u64* hi) {
    *lo = s.start + t_local * TILE;
    const u64 e = *lo + TILE, end = s.start + s.n;
    *hi = e < end ? e : end;
}

// L0: the input is the window array (canon + flags, invalid windows dropped); above: the keys of the partitions
template <bool L0>
__global__ void __launch_bounds__(CT) count_kernel(Seg* __restrict__ segs, const u32* __restrict__ tile_seg, const u64* __restrict__ in,
                                                   const uint8_t* __restrict__ flags, u64* __restrict__ hist) {
    __shared__ u32 h[RADIX];
    __shared__ unsigned long long red[2][CT / 64];
    const u32 si = L0 ? 0u : tile_seg[blockIdx.x];
    const Seg s = segs[si];
    const u64 t_local = blockIdx.x - s.tile_base, nt = ceil_div(s.n, TILE);
    const u32 w = digit_width(s.hi_bit), sh = s.hi_bit - w, mask = (1u << w) - 1u;
    h[threadIdx.x] = 0;
    __syncthreads();
    u64 lo, hi;
    tile_range(s, t_local, &lo, &hi);
    unsigned long long mn = ~0ull, mx = 0ull;
    for (u64 i = lo + threadIdx.x; i < hi; i += CT) {
        if (L0 && !(flags[i] & KMX_WIN_VALID)) continue;
        const unsigned long long key = in[i];
        atomicAdd(&h[(u32)(key >> sh) & mask], 1u);
        mn = key < mn ? key : mn;
        mx = key > mx ? key : mx;
    }
    for (u32 o = 32; o > 0; o >>= 1) {
        const unsigned long long a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63u) == 0) {
        red[0][threadIdx.x >> 6] = mn;
        red[1][threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    hist[s.tile_base * RADIX + (u64)threadIdx.x * nt + t_local] = h[threadIdx.x];
    if (threadIdx.x == 0) {
        for (u32 j = 1; j < CT / 64; ++j) {
            mn = red[0][j] < mn ? red[0][j] : mn;
            mx = red[1][j] > mx ? red[1][j] : mx;
        }
        if (mn != ~0ull) atomicMin(&segs[si].mn, mn);
        if (mx != 0ull) atomicMax(&segs[si].mx, mx);
    }
}

// a block per (partition, digit): the digit's per-tile counts -> exclusive prefix; the digit's total -> coltot.  Level 0: its one
// partition; above: the partitions of more than COL_SERIAL tiles, listed in `big` (a heavy hitter's partition holds most of the batch)
__global__ void __launch_bounds__(CT) colscan_kernel(const Seg* __restrict__ segs, const u32* __restrict__ big, u64* __restrict__ hist,
                                                     u64* __restrict__ coltot) {
    __shared__ u64 sh[CT];
    const u32 si = big ? big[blockIdx.x / RADIX] : blockIdx.x / RADIX, b = blockIdx.x % RADIX;
    const Seg s = segs[si];
    const u64 nt = ceil_div(s.n, TILE);
    u64 tot;
    block_scan_array(hist + s.tile_base * RADIX + (u64)b * nt, nt, sh, &tot);
    if (threadIdx.x == 0) coltot[(u64)si * RADIX + b] = tot;
}

// levels above 0: a block per partition of at most COL_SERIAL tiles, a thread per digit walking its column (longer ones: above)
__global__ void __launch_bounds__(CT) colscan_seg_kernel(const Seg* __restrict__ segs, u64* __restrict__ hist, u64* __restrict__ coltot) {
    const Seg s = segs[blockIdx.x];
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

// a block per partition: the digit totals -> the children's bases (in coltot, relative to the partition's start); the
// partition's runs if it needs no scatter; else its children to the next level and the leaf groups
__global__ void __launch_bounds__(CT) segfinal_kernel(Seg* __restrict__ segs, u64* __restrict__ coltot, Seg* __restrict__ next, u64 max_next,
                                                      u32* __restrict__ big, u64 max_big,
                                                      Leaf* __restrict__ leaves, u64 max_leaf, Leaf* __restrict__ small, u64 max_small,
                                                      Counters* __restrict__ cnt, u32 dst_is_keys,
                                                      u64* __restrict__ keys, u64* __restrict__ other, uint8_t* __restrict__ keep, u32 level0) {
    __shared__ u64 sh[CT];
    const u32 si = blockIdx.x;
    const Seg s = segs[si];
    const u64 v = coltot[(u64)si * RADIX + threadIdx.x];
    u64 total;
    const u64 base = block_exscan(v, sh, &total);
    coltot[(u64)si * RADIX + threadIdx.x] = base;
    if (level0 && threadIdx.x == 0) cnt->n_valid = total;
    if (total == 0) {
        if (threadIdx.x == 0) segs[si].skip = 1u;
        return;
    }
    const u32 w = digit_width(s.hi_bit), shift = s.hi_bit - w;
    if (s.mn == s.mx) {   // one key: one run
        if (threadIdx.x == 0) {
            keys[s.start] = s.mn;
            other[s.start] = total;
            keep[s.start] = 1u;
            segs[si].skip = 1u;
        }
        return;
    }
    if (shift == 0) {     // the last digit: every bucket is one key
        if (v != 0) {
            const u64 key = ((s.mn >> w) << w) | threadIdx.x;
            keys[s.start + base] = key;
            other[s.start + base] = v;
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
                    next[i_nx] = Seg{sb, nb, i_tile, ~0ull, 0ull, shift, 0u};
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
__global__ void __launch_bounds__(CT) scatter_kernel(const Seg* __restrict__ segs, const u32* __restrict__ tile_seg, const u64* __restrict__ in,
                                                     const uint8_t* __restrict__ flags, const u64* __restrict__ hist,
                                                     const u64* __restrict__ coltot, u64* __restrict__ out) {
    __shared__ u64 pos[RADIX];
    __shared__ u32 fill[RADIX];
    const u32 si = L0 ? 0u : tile_seg[blockIdx.x];
    const Seg s = segs[si];
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
        const u64 key = in[i];
        const u32 d = (u32)(key >> sh) & mask;
        out[pos[d] + atomicAdd(&fill[d], 1u)] = key;
    }
}

// level 0: one partition, the whole window array
__global__ void seg_init_kernel(Seg* __restrict__ segs, u64 n_win, u32 hi_bit) { segs[0] = Seg{0u, n_win, 0u, ~0ull, 0ull, hi_bit, 0u}; }

// the tiles of the next level's partitions -> their partition
__global__ void __launch_bounds__(CT) tilemap_kernel(const Seg* __restrict__ segs, u32* __restrict__ tile_seg) {
    const Seg s = segs[blockIdx.x];
    const u64 nt = ceil_div(s.n, TILE);
    for (u64 j = threadIdx.x; j < nt; j += CT) tile_seg[s.tile_base + j] = blockIdx.x;
}

// a block per leaf group of at most CAP keys: bitonic sort in LDS, run-length encoding
template <u32 CAP>
__global__ void __launch_bounds__(CT) leaf_kernel(const Leaf* __restrict__ leaves, u64* __restrict__ keys, u64* __restrict__ other,
                                                  uint8_t* __restrict__ keep) {
    __shared__ u64 a[CAP];
    __shared__ uint16_t head_at[CAP];
    __shared__ u64 sh[CT];
    const Leaf L = leaves[blockIdx.x];
    const u32 n = (u32)L.n;
    const u64* src = L.in_keys ? keys : other;
    u32 P = 2;
    while (P < n) P <<= 1;
    for (u32 i = threadIdx.x; i < P; i += CT) a[i] = i < n ? src[L.start + i] : ~0ull;
    for (u32 size = 2; size <= P; size <<= 1) {
        for (u32 stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (u32 t = threadIdx.x; t < (P >> 1); t += CT) {
                const u32 i = 2u * t - (t & (stride - 1u)), j = i + stride;
                const bool up = (i & size) == 0;
                const u64 x = a[i], y = a[j];
                if ((x > y) == up) {
                    a[i] = y;
                    a[j] = x;
                }
            }
        }
    }
    __syncthreads();
    // run heads: thread t looks at positions [16 t, 16 t + 16)
    constexpr u32 PER = CAP / CT;
    const u32 i0 = threadIdx.x * PER;
    u32 heads = 0;
    for (u32 j = 0; j < PER; ++j) {
        const u32 i = i0 + j;
        if (i < n && (i == 0 || a[i] != a[i - 1u])) ++heads;
    }
    u64 nd;
    u32 r = (u32)block_exscan(heads, sh, &nd);
    for (u32 j = 0; j < PER; ++j) {
        const u32 i = i0 + j;
        if (i < n && (i == 0 || a[i] != a[i - 1u])) head_at[r++] = (uint16_t)i;
    }
    __syncthreads();
    for (u32 q = threadIdx.x; q < (u32)nd; q += CT) {
        const u32 p = head_at[q], e = q + 1u < (u32)nd ? (u32)head_at[q + 1u] : n;
        keys[L.start + q] = a[p];
        other[L.start + q] = e - p;
        keep[L.start + q] = 1u;
    }
}

// ---------------------------------------------------------------- compaction of the kept entries
// a wave per quarter of the block's positions, 64 at a time: the ballot of the kept bytes gives each lane its slot
__global__ void __launch_bounds__(CT) keep_write_kernel(const uint8_t* __restrict__ keep, const u64* __restrict__ partial, const u64* __restrict__ keys,
                                                        const u64* __restrict__ counts, u64* __restrict__ out_k, u64* __restrict__ out_c) {
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
            out_c[r] = counts[i];
        }
        o += (u64)__popcll(m);
    }
}

// ---------------------------------------------------------------- merge of two tables
// merge path: thread t writes outputs [8 t, 8 t + 8); on equal keys the item of `a` goes first
__global__ void __launch_bounds__(CT) merge_kernel(const u64* __restrict__ ka, const u64* __restrict__ ca, u64 na, const u64* __restrict__ kb,
                                                   const u64* __restrict__ cb, u64 nb, u64* __restrict__ mk, u64* __restrict__ mc) {
    const u64 n = na + nb, d = ((u64)blockIdx.x * CT + threadIdx.x) * MERGE_IPT;
    if (d >= n) return;
    u64 lo = d > nb ? d - nb : 0u, hi = d < na ? d : na;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (ka[mid] <= kb[d - 1u - mid]) lo = mid + 1u;
        else hi = mid;
    }
    u64 i = lo, j = d - lo;
    for (u32 q = 0; q < MERGE_IPT && d + q < n; ++q) {
        if (j >= nb || (i < na && ka[i] <= kb[j])) {
            mk[d + q] = ka[i];
            mc[d + q] = ca[i];
            ++i;
        } else {
            mk[d + q] = kb[j];
            mc[d + q] = cb[j];
            ++j;
        }
    }
}

__device__ __forceinline__ bool is_head(const u64* mk, u64 i) { return i == 0 || mk[i] != mk[i - 1u]; }

__global__ void __launch_bounds__(CT) head_count_kernel(const u64* __restrict__ mk, u64 n, u64* __restrict__ partial) {
    __shared__ u64 sh[CT];
    const u64 i0 = (u64)blockIdx.x * MCHUNK + (u64)threadIdx.x * 16u;
    u64 c = 0;
    for (u32 j = 0; j < 16; ++j)
        if (i0 + j < n && is_head(mk, i0 + j)) ++c;
    u64 tot;
    (void)block_exscan(c, sh, &tot);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(CT) head_write_kernel(const u64* __restrict__ mk, const u64* __restrict__ mc, u64 n, const u64* __restrict__ partial,
                                                        u64* __restrict__ out_k, u64* __restrict__ out_c) {
    __shared__ u64 sh[CT];
    const u64 i0 = (u64)blockIdx.x * MCHUNK + (u64)threadIdx.x * 16u;
    u64 c = 0;
    for (u32 j = 0; j < 16; ++j)
        if (i0 + j < n && is_head(mk, i0 + j)) ++c;
    u64 tot;
    u64 o = partial[blockIdx.x] + block_exscan(c, sh, &tot);
    for (u32 j = 0; j < 16; ++j) {
        const u64 i = i0 + j;
        if (i < n && is_head(mk, i)) {
            // (each table holds a key once: an equal neighbour is the other table's entry)
            out_k[o] = mk[i];
            out_c[o] = mc[i] + (i + 1u < n && mk[i + 1u] == mk[i] ? mc[i + 1u] : 0u);
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
// The work area of one count, after the canon / flags arrays: keys (8 B per window), keep (1 B per window), then the
// level arrays.  `n` = the windows the area is sized for.
struct CountArea {
    u64* keys;
    uint8_t* keep;
    u64* hist;
    u64* coltot;
    u32* tile_seg;
    u32* big;
    Seg* segs[2];
    Leaf* leaves;
    Leaf* small;
    u64* partial;
    Counters* cnt;
    size_t keep_bytes;
};

size_t area_layout(u64 n, CountArea* out, void* base) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += align256(bytes);
        return base ? static_cast<char*>(base) + at : nullptr;
    };
    CountArea a{};
    a.keys = reinterpret_cast<u64*>(take(8u * n));
    a.keep_bytes = ceil_div(n, CHUNK) * CHUNK;
    a.keep = reinterpret_cast<uint8_t*>(take(a.keep_bytes));
    a.hist = reinterpret_cast<u64*>(take(8u * RADIX * max_tiles(n)));
    a.coltot = reinterpret_cast<u64*>(take(8u * RADIX * max_segs(n)));
    a.tile_seg = reinterpret_cast<u32*>(take(4u * max_tiles(n)));
    a.big = reinterpret_cast<u32*>(take(4u * max_big(n)));
    a.segs[0] = reinterpret_cast<Seg*>(take(sizeof(Seg) * max_segs(n)));
    a.segs[1] = reinterpret_cast<Seg*>(take(sizeof(Seg) * max_segs(n)));
    a.leaves = reinterpret_cast<Leaf*>(take(sizeof(Leaf) * max_leaves(n)));
    a.small = reinterpret_cast<Leaf*>(take(sizeof(Leaf) * max_small_leaves(n)));
    a.partial = reinterpret_cast<u64*>(take(8u * (ceil_div(n, CHUNK) + 2u)));
    a.cnt = reinterpret_cast<Counters*>(take(sizeof(Counters)));
    if (out) *out = a;
    return off;
}

}  // namespace

size_t count_area_bytes(u64 n) { return area_layout(n, nullptr, nullptr); }

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
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = hipMemcpyAsync(h_pinned, wo + n_reads, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    *wo_out = wo;
    *h_total = h_pinned[0];
    return hipSuccess;
}

// Sort and tally the n_win windows (canon / flags) of a batch of k-mers; the table is left in `area` (keys in a.keys, counts
// in canon, marked in a.keep) and its size comes back in *h_distinct.  Synchronous: one host round trip per level and one
// for the number of distinct keys.  *bad: the level arrays overflowed their bounds (a bug, never expected).
hipError_t launch_count_sort(u64* canon, const uint8_t* flags, u64 n_win, u32 k, void* area, unsigned long long* h_pinned, u64* h_valid,
                             u64* h_distinct, bool* bad, hipStream_t st) {
    CountArea a;
    area_layout(n_win, &a, area);
    *bad = false;
    hipError_t e;
    if ((e = hipMemsetAsync(a.keep, 0, a.keep_bytes, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(seg_init_kernel, dim3(1), dim3(1), 0, st, a.segs[0], n_win, 2u * k);
    const u64 ms = max_segs(n_win), ml = max_leaves(n_win), mls = max_small_leaves(n_win), mt = max_tiles(n_win), mb = max_big(n_win);
    u64 n_seg = 1, n_tiles = ceil_div(n_win, TILE), n_big = 0;
    *h_valid = 0;
    for (u32 level = 0; n_seg != 0; ++level) {
        if (level > 8u) {   // (2k <= 62 bits: at most 8 digits)
            *bad = true;
            return hipSuccess;
        }
        const bool l0 = level == 0;
        Seg* cur = a.segs[level & 1u];
        Seg* nxt = a.segs[(level & 1u) ^ 1u];
        // level 0 reads the windows (canon) and writes `keys`; then the levels alternate
        const bool src_is_keys = (level & 1u) == 1u;
        u64* src = src_is_keys ? a.keys : canon;
        u64* dst = src_is_keys ? canon : a.keys;
        if ((e = hipMemsetAsync(a.cnt, 0, LEVEL_COUNTERS, st)) != hipSuccess) return e;
        if (l0) hipLaunchKernelGGL(count_kernel<true>, dim3((unsigned)n_tiles), dim3(CT), 0, st, cur, a.tile_seg, src, flags, a.hist);
        else hipLaunchKernelGGL(count_kernel<false>, dim3((unsigned)n_tiles), dim3(CT), 0, st, cur, a.tile_seg, src, flags, a.hist);
        if (l0) {
            hipLaunchKernelGGL(colscan_kernel, dim3(RADIX), dim3(CT), 0, st, cur, (const u32*)nullptr, a.hist, a.coltot);
        } else {
            hipLaunchKernelGGL(colscan_seg_kernel, dim3((unsigned)n_seg), dim3(CT), 0, st, cur, a.hist, a.coltot);
            if (n_big) hipLaunchKernelGGL(colscan_kernel, dim3((unsigned)(n_big * RADIX)), dim3(CT), 0, st, cur, (const u32*)a.big, a.hist, a.coltot);
        }
        hipLaunchKernelGGL(segfinal_kernel, dim3((unsigned)n_seg), dim3(CT), 0, st, cur, a.coltot, nxt, ms, a.big, mb, a.leaves, ml, a.small, mls, a.cnt,
                           src_is_keys ? 0u : 1u, a.keys, canon, a.keep, l0 ? 1u : 0u);
        if (l0) hipLaunchKernelGGL(scatter_kernel<true>, dim3((unsigned)n_tiles), dim3(CT), 0, st, cur, a.tile_seg, src, flags, a.hist, a.coltot, dst);
        else hipLaunchKernelGGL(scatter_kernel<false>, dim3((unsigned)n_tiles), dim3(CT), 0, st, cur, a.tile_seg, src, flags, a.hist, a.coltot, dst);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(h_pinned, a.cnt, LEVEL_COUNTERS, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
        if (l0) *h_valid = h_pinned[0];
        const u64 n_next = h_pinned[1], n_next_tiles = h_pinned[2], n_leaf = h_pinned[3], n_small = h_pinned[5], n_next_big = h_pinned[6];
        if (h_pinned[4] != 0 || n_next > ms || n_leaf > ml || n_small > mls || n_next_tiles > mt || n_next_big > mb) {
            *bad = true;
            return hipSuccess;
        }
        if (n_leaf) hipLaunchKernelGGL(leaf_kernel<LEAF>, dim3((unsigned)n_leaf), dim3(CT), 0, st, a.leaves, a.keys, canon, a.keep);
        if (n_small) hipLaunchKernelGGL(leaf_kernel<LEAF_SMALL>, dim3((unsigned)n_small), dim3(CT), 0, st, a.small, a.keys, canon, a.keep);
        if (n_next) hipLaunchKernelGGL(tilemap_kernel, dim3((unsigned)n_next), dim3(CT), 0, st, nxt, a.tile_seg);
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

// the table launch_count_sort left in `area` -> out_k / out_c (n_distinct entries)
hipError_t launch_count_emit(const u64* canon, u64 n_win, u64 n_valid, void* area, u64* out_k, u64* out_c, hipStream_t st) {
    CountArea a;
    area_layout(n_win, &a, area);
    const u64 nb = ceil_div(n_valid, CHUNK);
    if (nb) hipLaunchKernelGGL(keep_write_kernel, dim3((unsigned)nb), dim3(CT), 0, st, a.keep, a.partial, a.keys, canon, out_k, out_c);
    return hipGetLastError();
}

size_t count_merge_bytes(u64 n) { return 2u * align256(8u * n) + align256(8u * (ceil_div(n, MCHUNK) + 2u)); }

// merge of two tables into `area` and the number of distinct keys of the union (synchronous: one host round trip)
hipError_t launch_count_merge(const u64* ka, const u64* ca, u64 na, const u64* kb, const u64* cb, u64 nb, void* area, unsigned long long* h_pinned,
                              u64* h_out, hipStream_t st) {
    const u64 n = na + nb;
    u64* mk = static_cast<u64*>(area);
    u64* mc = reinterpret_cast<u64*>(static_cast<char*>(area) + align256(8u * n));
    u64* partial = reinterpret_cast<u64*>(static_cast<char*>(area) + 2u * align256(8u * n));
    const u64 nblk = ceil_div(n, MCHUNK);
    hipLaunchKernelGGL(merge_kernel, dim3((unsigned)ceil_div(n, (u64)CT * MERGE_IPT)), dim3(CT), 0, st, ka, ca, na, kb, cb, nb, mk, mc);
    hipLaunchKernelGGL(head_count_kernel, dim3((unsigned)nblk), dim3(CT), 0, st, mk, n, partial);
    hipLaunchKernelGGL(scan_single_kernel, dim3(1), dim3(CT), 0, st, partial, nblk, partial + nblk);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = hipMemcpyAsync(h_pinned, partial + nblk, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    *h_out = h_pinned[0];
    return hipSuccess;
}

hipError_t launch_count_merge_emit(u64 n, const void* area, u64* out_k, u64* out_c, hipStream_t st) {
    const u64* mk = static_cast<const u64*>(area);
    const u64* mc = reinterpret_cast<const u64*>(static_cast<const char*>(area) + align256(8u * n));
    const u64* partial = reinterpret_cast<const u64*>(static_cast<const char*>(area) + 2u * align256(8u * n));
    const u64 nblk = ceil_div(n, MCHUNK);
    hipLaunchKernelGGL(head_write_kernel, dim3((unsigned)nblk), dim3(CT), 0, st, mk, mc, n, partial, out_k, out_c);
    return hipGetLastError();
}

}  // namespace kmx
