// kmx_sketch.hip -- the counting sketch: kmx_sketch_add(2) / kmx_sketch_add_words(2), kmx_sketch_lookup(2) / kmx_sketch_lookup_reads(2),
// kmx_sketch_merge, kmx_sketch_stats and the filter step of kmx_count_canonical_min(2).  kmx.h has the contract (layout, key hash,
// the saturating add, the estimate); DESIGN 4.6.21 has the reasoning.
//
// A blocked count-min sketch of saturating bytes: a key owns one 64-byte block -- four rows of 16 cells, one cache line -- and one
// cell in each row.  One lane per key in a grid-stride loop over (keys, flags); no LDS, no work buffer, no scratch.
//   add     Per row: the aligned dword that holds the cell is read, and unless the cell already holds 255 the dword goes back through
//           a compare-and-swap with that one byte replaced by min(255, cell + w).  The three neighbours in the dword belong to other
//           counters: the swap carries them unchanged, so no carry ever reaches them, and a swap that lost against a neighbour's
//           update is tried again on the word it returned.  A cell only grows and a saturating add commutes, so after any set of adds
//           in any order a cell holds min(255, the sum of its weights): launch shape and arrival order leave no trace.  Reading first
//           is what keeps homopolymer and repeat k-mers cheap: a saturated cell costs one load and no atomic.
//   lookup  The four bytes of the key's line, their minimum.  The filter of kmx_count_canonical_min(2) is the same read: it clears
//           KMX_WIN_VALID where the minimum is below the threshold.
//   merge   Cellwise min(255, a + b), sixteen cells a lane by SWAR on the even and the odd bytes; a lane reads its sixteen bytes of
//           both inputs before it writes them, so the output may be either input.
//   stats   The values of the cells, tallied in block-private LDS words (a block sees fewer than 2^32 cells) with the zero cells --
//           most of a well-sized sketch -- counted in registers and added once per wave; one device atomic per non-empty bin.
// Vector loads, vector stores and integer device atomics only.
#include "kmx_key_hash.h"   // (the key hash and the sweep's grid: shared with kmx_hll.hip)

namespace kmx {

namespace {

constexpr u32 SK_STATS_IPT = 4;   // uint4 pieces per thread and grid step of the stats

// byte offset of the key's block (no shift by 64: log2_blocks = 0 is one block)
__device__ __forceinline__ u64 block_at(u64 h, u32 log2_blocks) { return log2_blocks ? (h >> (64u - log2_blocks)) << 6 : 0ull; }
// byte offset, inside the block, of the key's cell in row j
__device__ __forceinline__ u32 cell_in(u64 h, u32 j) { return 16u * j + ((u32)(h >> (4u * j)) & 15u); }

// min(255, cell + w) into one byte of an aligned dword, the other three carried unchanged
__device__ __forceinline__ void cell_add(uint8_t* sketch, u64 at, u32 w) {
    u32* const p = reinterpret_cast<u32*>(sketch + (at & ~3ull));
    const u32 sh = 8u * ((u32)at & 3u);
    u32 old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        const u32 c = (old >> sh) & 255u;
        if (c == 255u) return;
        const u32 s = c + w < 255u ? c + w : 255u;   // (w <= 255)
        const u32 want = (old & ~(255u << sh)) | (s << sh);
        if (__hip_atomic_compare_exchange_strong(p, &old, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    }
}

// the estimate of a key: the minimum of its four cells
__device__ __forceinline__ u32 estimate(const uint8_t* __restrict__ sketch, u64 h, u32 log2_blocks) {
    const uint8_t* const b = sketch + block_at(h, log2_blocks);
    u32 c[4];
#pragma unroll
    for (u32 j = 0; j < 4; ++j) c[j] = b[cell_in(h, j)];
    const u32 x = c[0] < c[1] ? c[0] : c[1], y = c[2] < c[3] ? c[2] : c[3];
    return x < y ? x : y;
}

// weights == nullptr: 1 each; flags == nullptr: every key counts, otherwise those with KMX_WIN_VALID
template <u32 W>
__global__ void __launch_bounds__(CT) sketch_add_kernel(const u64* __restrict__ keys, const u64* __restrict__ weights,
                                                        const uint8_t* __restrict__ flags, u64 n, uint8_t* sketch, u32 log2_blocks, u64 seed) {
    const u64 stride = (u64)gridDim.x * CT;
    for (u64 i = (u64)blockIdx.x * CT + threadIdx.x; i < n; i += stride) {
        if (flags != nullptr && (flags[i] & KMX_WIN_VALID) == 0u) continue;
        u32 w = 1u;
        if (weights != nullptr) {
            const u64 x = weights[i];
            w = x < 255u ? (u32)x : 255u;
            if (w == 0u) continue;
        }
        const u64 h = key_hash<W>(Key<W>::load(keys, i), seed);
        const u64 b = block_at(h, log2_blocks);
#pragma unroll
        for (u32 j = 0; j < 4; ++j) cell_add(sketch, b + cell_in(h, j), w);
    }
}

template <u32 W>
__global__ void __launch_bounds__(CT) sketch_lookup_kernel(const u64* __restrict__ keys, const uint8_t* __restrict__ flags, u64 n,
                                                           const uint8_t* __restrict__ sketch, u32 log2_blocks, u64 seed,
                                                           uint8_t* __restrict__ est) {
    const u64 stride = (u64)gridDim.x * CT;
    for (u64 i = (u64)blockIdx.x * CT + threadIdx.x; i < n; i += stride) {
        u32 e = 0u;
        if (flags == nullptr || (flags[i] & KMX_WIN_VALID) != 0u) e = estimate(sketch, key_hash<W>(Key<W>::load(keys, i), seed), log2_blocks);
        est[i] = (uint8_t)e;
    }
}

// clears KMX_WIN_VALID of every window whose estimate is below min_est (1 <= min_est <= 255)
template <u32 W>
__global__ void __launch_bounds__(CT) sketch_filter_kernel(const u64* __restrict__ keys, uint8_t* __restrict__ flags, u64 n,
                                                           const uint8_t* __restrict__ sketch, u32 log2_blocks, u64 seed, u32 min_est) {
    const u64 stride = (u64)gridDim.x * CT;
    for (u64 i = (u64)blockIdx.x * CT + threadIdx.x; i < n; i += stride) {
        const u32 f = flags[i];
        if ((f & KMX_WIN_VALID) == 0u) continue;
        if (estimate(sketch, key_hash<W>(Key<W>::load(keys, i), seed), log2_blocks) < min_est) flags[i] = (uint8_t)(f & ~(u32)KMX_WIN_VALID);
    }
}

// bytewise min(255, a + b) of four cells: the even and the odd bytes in 16-bit fields, a field's bit 8 spread over its low byte
__device__ __forceinline__ u32 sat_add4(u32 a, u32 b) {
    u32 e = (a & 0x00FF00FFu) + (b & 0x00FF00FFu), o = ((a >> 8) & 0x00FF00FFu) + ((b >> 8) & 0x00FF00FFu);
    const u32 ce = e & 0x01000100u, co = o & 0x01000100u;
    e = (e | (ce - (ce >> 8))) & 0x00FF00FFu;
    o = (o | (co - (co >> 8))) & 0x00FF00FFu;
    return e | (o << 8);
}

// (no __restrict__: out may be a or b)
__global__ void __launch_bounds__(CT) sketch_merge_kernel(const uint4* a, const uint4* b, u64 n16, uint4* out) {
    const u64 stride = (u64)gridDim.x * CT;
    for (u64 i = (u64)blockIdx.x * CT + threadIdx.x; i < n16; i += stride) {
        const uint4 x = a[i], y = b[i];
        out[i] = make_uint4(sat_add4(x.x, y.x), sat_add4(x.y, y.y), sat_add4(x.z, y.z), sat_add4(x.w, y.w));
    }
}

// the number of zero bytes of a dword
__device__ __forceinline__ u32 zero_bytes(u32 v) {
    const u32 nz = ((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v;   // bit 7 of a byte: the byte is not zero
    return 4u - (u32)__popc(nz & 0x80808080u);
}

__global__ void __launch_bounds__(CT) sketch_stats_kernel(const uint4* __restrict__ cells, u64 n16, u64 per_block, unsigned long long* hist) {
    __shared__ u32 bins[256];
    bins[threadIdx.x] = 0u;   // (CT == 256)
    __syncthreads();
    const u64 lo = (u64)blockIdx.x * per_block, hi = lo + per_block < n16 ? lo + per_block : n16;
    u64 zeros = 0;
    for (u64 i = lo + threadIdx.x; i < hi; i += CT) {
        const uint4 v = cells[i];
        const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (u32 q = 0; q < 4; ++q) {
            const u32 z = zero_bytes(w[q]);
            zeros += z;
            if (z == 4u) continue;
#pragma unroll
            for (u32 s = 0; s < 32u; s += 8u) {
                const u32 c = (w[q] >> s) & 255u;
                if (c) atomicAdd(&bins[c], 1u);
            }
        }
    }
    zeros = wave_sum_shfl(zeros);
    if ((threadIdx.x & 63u) == 0u && zeros) atomicAdd(&hist[0], (unsigned long long)zeros);
    __syncthreads();
    const u32 c = bins[threadIdx.x];
    if (c) atomicAdd(&hist[threadIdx.x], (unsigned long long)c);
}
static_assert(CT == 256, "the stats kernel keeps one bin per thread");

}  // namespace

// ---------------------------------------------------------------- host side
hipError_t launch_sketch_add(u32 words, const u64* keys, const u64* weights, const uint8_t* flags, u64 n, uint8_t* sketch, u32 log2_blocks, u64 seed,
                             int n_cu, hipStream_t st) {
    if (n == 0) return hipSuccess;
    with_width(words, [&](auto w) {
        constexpr u32 W = decltype(w)::value;
        hipLaunchKernelGGL(sketch_add_kernel<W>, dim3(sweep_blocks(n, n_cu)), dim3(CT), 0, st, keys, weights, flags, n, sketch, log2_blocks, seed);
    });
    return hipGetLastError();
}

hipError_t launch_sketch_lookup(u32 words, const u64* keys, const uint8_t* flags, u64 n, const uint8_t* sketch, u32 log2_blocks, u64 seed,
                                uint8_t* est, int n_cu, hipStream_t st) {
    if (n == 0) return hipSuccess;
    with_width(words, [&](auto w) {
        constexpr u32 W = decltype(w)::value;
        hipLaunchKernelGGL(sketch_lookup_kernel<W>, dim3(sweep_blocks(n, n_cu)), dim3(CT), 0, st, keys, flags, n, sketch, log2_blocks, seed, est);
    });
    return hipGetLastError();
}

hipError_t launch_sketch_filter(u32 words, const u64* keys, uint8_t* flags, u64 n, const uint8_t* sketch, u32 log2_blocks, u64 seed, u32 min_est,
                                int n_cu, hipStream_t st) {
    if (n == 0) return hipSuccess;
    with_width(words, [&](auto w) {
        constexpr u32 W = decltype(w)::value;
        hipLaunchKernelGGL(sketch_filter_kernel<W>, dim3(sweep_blocks(n, n_cu)), dim3(CT), 0, st, keys, flags, n, sketch, log2_blocks, seed, min_est);
    });
    return hipGetLastError();
}

hipError_t launch_sketch_merge(const uint8_t* a, const uint8_t* b, u32 log2_blocks, uint8_t* out, int n_cu, hipStream_t st) {
    const u64 n16 = 4ull << log2_blocks;
    hipLaunchKernelGGL(sketch_merge_kernel, dim3(sweep_blocks(n16, n_cu)), dim3(CT), 0, st, reinterpret_cast<const uint4*>(a),
                       reinterpret_cast<const uint4*>(b), n16, reinterpret_cast<uint4*>(out));
    return hipGetLastError();
}

hipError_t launch_sketch_stats(const uint8_t* sketch, u32 log2_blocks, u64* hist, int n_cu, hipStream_t st) {
    const u64 n16 = 4ull << log2_blocks;
    // a block's share: whole steps of the block, and fewer than 2^32 cells (2^27 pieces of 16) so that its LDS bins cannot wrap
    u64 nb = ceil_div(n16, (u64)CT * SK_STATS_IPT);
    const u64 cap = (u64)(n_cu > 0 ? n_cu : 256) * 8u;
    if (nb > cap) nb = cap;
    u64 per_block = ceil_div(ceil_div(n16, nb), CT) * CT;
    if (per_block > (1ull << 27)) per_block = 1ull << 27;
    nb = ceil_div(n16, per_block);
    hipLaunchKernelGGL(sketch_stats_kernel, dim3((unsigned)nb), dim3(CT), 0, st, reinterpret_cast<const uint4*>(sketch), n16, per_block,
                       reinterpret_cast<unsigned long long*>(hist));
    return hipGetLastError();
}

}  // namespace kmx
