// kmx_count_common.h -- what the count family shares: kmx_count.hip (the counter and the merge, one source for one-word keys,
// k <= 31, and two-word keys, k = 33..64), kmx_count_query.hip, kmx_count_setop.hip, kmx_count_read_stats.hip and kmx_count_graph.hip
// (the query and the graph source through kmx_count_dir.h, the directory their searches share).  On the device: the
// key of W words (Key<W>: the one type every kernel of the family is templated on), block scans and the block sum, the records a
// level leaves for the host and for the leaf kernels, and the compaction of marked entries (the count of the marked bytes and the
// wave-ballot copy, compact_write_kernel: the counter's and the filter's).  On the host: the launchers' tail that brings one record
// back (read_back) and the dispatch on the key width (with_width).  Everything here has internal linkage (each translation unit
// compiles its own copy, as it did when kmx_count.hip was the only user).
#pragma once
#include <type_traits>

#include "kmx_device.h"
#include "kmx_launch.h"

namespace kmx {

namespace {

constexpr u32 CT = 256;                       // threads per block
constexpr u32 RBITS = 8, RADIX = 1u << RBITS; // digit width: 256 bins
constexpr u32 COL_SERIAL = 64;                // levels above 0: a column of at most this many tiles is scanned by one thread
constexpr u32 CHUNK = CT * 64;                // positions per block in the compaction passes
constexpr u32 MCHUNK = CT * 16;               // positions per block in the merge's collapse passes
constexpr u32 MERGE_IPT = 8;                  // merged items per thread

// ---------------------------------------------------------------- a key of W words
// One u64 for k <= 31; {lo, hi} for k = 33..64: one 16-byte element everywhere (the slot layout of kmx_canonical_windows2: a dwordx4
// access per lane in global memory, a b128 element in LDS), ordered as the 2k-bit integer -- high word first, then low.  Arrays of
// keys are passed as u64* (W words per key) and read and written through load / store.
template <u32 W> struct Key;
template <> struct Key<1> {
    u64 lo;
    __device__ __forceinline__ static Key load(const u64* a, u64 i) { return Key{a[i]}; }
    __device__ __forceinline__ static void store(u64* a, u64 i, const Key& v) { a[i] = v.lo; }
    __device__ __forceinline__ static void copy(u64* dst, u64 i, const u64* src, u64 j) { dst[i] = src[j]; }   // (element to element)
    __device__ __forceinline__ static Key sentinel() { return Key{~0ull}; }   // above every key: pads a leaf's sort
    // a run's count in the slot of the array that does not hold its key (read back as .lo)
    __device__ __forceinline__ static Key count(u64 c) { return Key{c}; }
    __device__ __forceinline__ bool less(const Key& o) const { return lo < o.lo; }
    __device__ __forceinline__ bool equal(const Key& o) const { return lo == o.lo; }
    __device__ __forceinline__ bool differs(const Key& o) const { return lo != o.lo; }
    __device__ __forceinline__ bool greater(const Key& o) const { return lo > o.lo; }
    // bits [sh, sh + 8) of the key at the bottom of the result (the caller masks): sh is uniform over the block
    __device__ __forceinline__ u32 bits(u32 sh) const { return (u32)(lo >> sh); }
    // the key with its lowest w bits (w <= 8) replaced by d
    __device__ __forceinline__ Key with_low(u32 w, u32 d) const { return Key{((lo >> w) << w) | d}; }
    // a bit at or above bit 2k: no key of a table has one (2k <= 62)
    __device__ __forceinline__ bool outside(u32 k) const { return (lo >> (2u * k)) != 0u; }
    // the top p bits of the 2k-bit key (0 < p <= 2k)
    __device__ __forceinline__ u64 prefix(u32 k, u32 p) const { return lo >> (2u * k - p); }
    // The key as a word of k bases (the graph layer, k >= 2): one base up with the top base dropped (Kmer::prepend_base with base 0),
    // one base down (Kmer::append_base before the new base goes in), the top base, base c at a top position that holds 0, and the
    // reverse complement (the element-wise kernels' revcomp_word).
    __device__ __forceinline__ Key shl_base(u32 k) const { return Key{(lo << 2) & mask2k(k)}; }
    __device__ __forceinline__ Key shr_base() const { return Key{lo >> 2}; }
    __device__ __forceinline__ u32 top_base(u32 k) const { return (u32)(lo >> (2u * k - 2u)) & 3u; }
    __device__ __forceinline__ Key with_top(u32 k, u32 c) const { return Key{lo | ((u64)c << (2u * k - 2u))}; }
    __device__ __forceinline__ Key revcomp(u32 k) const { return Key{revcomp_word(lo, k)}; }
};
template <> struct alignas(16) Key<2> {
    u64 lo, hi;
    __device__ __forceinline__ static Key load(const u64* a, u64 i) { return reinterpret_cast<const Key*>(a)[i]; }   // (one 16-byte load)
    __device__ __forceinline__ static void store(u64* a, u64 i, const Key& v) { reinterpret_cast<Key*>(a)[i] = v; }
    __device__ __forceinline__ static void copy(u64* dst, u64 i, const u64* src, u64 j) { reinterpret_cast<Key*>(dst)[i] = reinterpret_cast<const Key*>(src)[j]; }
    __device__ __forceinline__ static Key sentinel() { return Key{~0ull, ~0ull}; }
    __device__ __forceinline__ static Key count(u64 c) { return Key{c, 0u}; }
    __device__ __forceinline__ bool less(const Key& o) const { return hi < o.hi || (hi == o.hi && lo < o.lo); }
    // equal and differs are one question spelled twice, on purpose: `equal` is the compare the query and set-operation kernels were
    // built with (high word first), `differs` the one the counter's kernels were built with (word-wise xor, or).  The compiler keeps
    // the order of the two word compares it is given, so one spelling for both would change the instructions of one family.
    __device__ __forceinline__ bool equal(const Key& o) const { return hi == o.hi && lo == o.lo; }
    __device__ __forceinline__ bool differs(const Key& o) const { return ((lo ^ o.lo) | (hi ^ o.hi)) != 0; }
    __device__ __forceinline__ bool greater(const Key& o) const { return o.less(*this); }
    // (the field may straddle the two words: 2k mod 8 != 0)
    __device__ __forceinline__ u32 bits(u32 sh) const {
        if (sh >= 64u) return (u32)(hi >> (sh - 64u));
        if (sh == 0u) return (u32)lo;
        return (u32)((lo >> sh) | (hi << (64u - sh)));
    }
    __device__ __forceinline__ Key with_low(u32 w, u32 d) const { return Key{((lo >> w) << w) | d, hi}; }
    __device__ __forceinline__ bool outside(u32 k) const { return k < 64u && (hi >> (2u * k - 64u)) != 0u; }   // (k >= 33)
    // the field may straddle the word boundary: s = 2k - p bits lie below it, 36 <= s < 128
    __device__ __forceinline__ u64 prefix(u32 k, u32 p) const {
        const u32 s = 2u * k - p;
        return s >= 64u ? hi >> (s - 64u) : (hi << (64u - s)) | (lo >> s);
    }
    // (as above; the high word holds 2k - 64 bits, 2 .. 64 of them; the reverse complement is the 128-bit group reversal of the scans)
    __device__ __forceinline__ Key shl_base(u32 k) const {
        const u64 m = k >= 64u ? ~0ull : (1ull << (2u * k - 64u)) - 1ull;
        return Key{lo << 2, ((hi << 2) | (lo >> 62)) & m};
    }
    __device__ __forceinline__ Key shr_base() const { return Key{(lo >> 2) | (hi << 62), hi >> 2}; }
    __device__ __forceinline__ u32 top_base(u32 k) const { return (u32)(hi >> (2u * k - 66u)) & 3u; }
    __device__ __forceinline__ Key with_top(u32 k, u32 c) const { return Key{lo, hi | ((u64)c << (2u * k - 66u))}; }
    __device__ __forceinline__ Key revcomp(u32 k) const {
        const U128 r = lex_hash128(U128{~lo, ~hi}, k);
        return Key{r.lo, r.hi};
    }
};
static_assert(sizeof(Key<1>) == 8 && sizeof(Key<2>) == 16, "a key is one element of W words");

struct Leaf {
    u64 start, n;
    u32 in_keys;    // the group's keys are in `keys` (1) or in the other array (0)
    u32 pad;
};

// device counters of a level (one host read-back per level)
struct Counters {
    unsigned long long n_valid, n_next, n_next_tiles, n_leaf, overflow, n_leaf_small, n_next_big;
    u64 n_distinct;
};
constexpr size_t LEVEL_COUNTERS = 7u * 8u;   // (n_valid .. n_next_big: cleared before and read back after every level)
static_assert(LEVEL_COUNTERS <= KMX_PIN_BYTES, "the level counters are read back into the context's pinned words");

__host__ __device__ __forceinline__ u64 ceil_div(u64 a, u64 b) { return (a + b - 1u) / b; }
__device__ __forceinline__ u32 digit_width(u32 hi_bit) { return hi_bit < RBITS ? hi_bit : RBITS; }

// exclusive scan of one value per thread over the block (256 threads); *total = the sum; `sh` holds CT u64
__device__ __forceinline__ u64 block_exscan(u64 v, u64* sh, u64* total) {
    const u32 t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (u32 d = 1; d < CT; d <<= 1) {
        const u64 x = t >= d ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    *total = sh[CT - 1];
    const u64 ex = sh[t] - v;
    __syncthreads();
    return ex;
}

// exclusive scan in place of a[0..n) by one block, 8 contiguous entries per thread and step; *total = the sum
__device__ void block_scan_array(u64* a, u64 n, u64* sh, u64* total) {
    u64 carry = 0;
    for (u64 base = 0; base < n; base += (u64)CT * 8u) {
        const u64 i0 = base + (u64)threadIdx.x * 8u;
        u64 v[8], s = 0;
#pragma unroll
        for (u32 j = 0; j < 8; ++j) {
            v[j] = i0 + j < n ? a[i0 + j] : 0u;
            s += v[j];
        }
        u64 tot;
        u64 run = carry + block_exscan(s, sh, &tot);
#pragma unroll
        for (u32 j = 0; j < 8; ++j) {
            if (i0 + j < n) a[i0 + j] = run;
            run += v[j];
        }
        carry += tot;
    }
    *total = carry;
}

// the shuffle sum the set-operation kernels were built with: the DPP wave_sum of kmx_device.h is not timed in them yet
__device__ __forceinline__ u64 wave_sum_shfl(u64 v) {
#pragma unroll
    for (u32 o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum of one value per thread over the block, valid in thread 0; `sh` holds CT / 64 u64
__device__ __forceinline__ u64 block_sum(u64 v, u64* sh) {
    v = wave_sum_shfl(v);
    if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 t = 0;
    if (threadIdx.x == 0)
        for (u32 w = 0; w < CT / 64u; ++w) t += sh[w];
    __syncthreads();
    return t;
}

__global__ void __launch_bounds__(CT) scan_single_kernel(u64* __restrict__ a, u64 n, u64* __restrict__ total) {
    __shared__ u64 sh[CT];
    u64 t;
    block_scan_array(a, n, sh, &t);
    if (threadIdx.x == 0) *total = t;
}

// ---------------------------------------------------------------- compaction of the kept entries
__device__ __forceinline__ u32 kept_in(const uint8_t* keep, u64 i0) {
    const uint4* p = reinterpret_cast<const uint4*>(keep + i0);
    u32 c = 0;
#pragma unroll
    for (u32 j = 0; j < 4; ++j) {
        const uint4 v = p[j];
        c += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);   // (bytes are 0 or 1)
    }
    return c;
}

__global__ void __launch_bounds__(CT) keep_count_kernel(const uint8_t* __restrict__ keep, u64* __restrict__ partial) {
    __shared__ u64 sh[CT];
    u64 tot;
    (void)block_exscan(kept_in(keep, (u64)blockIdx.x * CHUNK + (u64)threadIdx.x * 64u), sh, &tot);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// The copy: a wave per quarter of the block's positions, 64 at a time: the ballot of the kept bytes gives each lane its slot.  A
// count is the low word of a slot of CW words: the counter leaves a run's count in a key-sized slot (CW = W, Key<W>::count), a
// table holds plain u64 (CW = 1, the filter).
template <u32 W, u32 CW>
__global__ void __launch_bounds__(CT) compact_write_kernel(const uint8_t* __restrict__ keep, const u64* __restrict__ partial,
                                                           const u64* __restrict__ keys, const u64* __restrict__ counts, u64* __restrict__ out_k,
                                                           u64* __restrict__ out_c) {
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
            Key<W>::store(out_k, r, Key<W>::load(keys, i));
            out_c[r] = Key<CW>::load(counts, i).lo;
        }
        o += (u64)__popcll(m);
    }
}

// ---------------------------------------------------------------- host side
// The tail of a launcher that needs one record on the host: the launches' error, then n_words u64 at d_src through the context's
// pinned words into h_out.  Synchronous: one host round trip.
hipError_t read_back(unsigned long long* h_pinned, const void* d_src, u32 n_words, u64* h_out, hipStream_t st) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = hipMemcpyAsync(h_pinned, d_src, 8u * n_words, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    for (u32 q = 0; q < n_words; ++q) h_out[q] = h_pinned[q];
    return hipSuccess;
}

// f(std::integral_constant<u32, words>{}), words = 1 or 2: the one place a launcher turns `words` into the W of its kernels
template <typename F>
auto with_width(u32 words, F&& f) {
    return words == 1u ? f(std::integral_constant<u32, 1>{}) : f(std::integral_constant<u32, 2>{});
}

}  // namespace

}  // namespace kmx
