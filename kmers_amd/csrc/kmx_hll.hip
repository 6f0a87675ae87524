// kmx_hll.hip -- the distinct-key estimator: kmx_hll_add(2) / kmx_hll_add_words(2), kmx_hll_merge, kmx_hll_stats.  kmx.h has the
// contract (registers, key hash, the update, the estimate from the bins); DESIGN 4.6.24 has the reasoning.
//
// HyperLogLog registers: 1 << p bytes, a key's hash names one (its top p bits) and a rank (1 + the leading zeros of the rest), and the
// register keeps the largest rank it has seen.  A maximum commutes and is idempotent, so the bytes depend on the set of keys alone.
// One lane per key in a grid-stride loop over (keys, flags), as the sketch's add; no work buffer, no scratch.
//   add     After a short warm-up almost no key raises its register, so every update reads first and takes an atomic only where its
//           rank is larger: the aligned dword that holds the register goes back through a compare-and-swap with that one byte replaced,
//           the three neighbours carried unchanged (the sketch's cell_add with max for the saturating add); a swap that lost is tried
//           again on the word it returned, and stops as soon as the byte there is large enough.  Two routes, chosen on the host
//           (launch_hll_add), the same bytes from both:
//             block-private  p <= HLL_LDS_MAX_LOG2_REGS and at least one key for every dword a block has to flush: the registers are
//                            a zeroed LDS array, the loop above runs on its dwords at workgroup scope, and at exit every lane walks
//                            dwords of it -- a zero dword is skipped, the others are folded into the global dword as a bytewise maximum,
//                            swapped in only where that differs from what is there.
//             global         the loop above on the global dword, at agent scope.
//   merge   Bytewise max(a, b), sixteen registers a lane by SWAR on the even and the odd bytes; a lane reads its sixteen bytes of both
//           inputs before it writes them, so the output may be either input.
//   stats   The values of the registers tallied in block-private LDS words, 64 bins an array: of a, and with b also of b and of
//           max(a, b), so a comparison reads each array once and writes no third one.  Zero registers are counted in registers and
//           added once per wave; one device atomic per non-empty bin.
// Vector loads, vector stores and integer atomics only; the device never touches a float (the estimate is the host's, from the bins).
#include "kmx_key_hash.h"

namespace kmx {

namespace {

// The cut-over of the add.  The block-private route keeps 1 << p bytes of LDS per block: 16 KiB at the cut, ten such
// blocks on a compute unit's 160 KiB.  It pays once a block has a key for every dword it flushes: below that the flush alone touches
// global memory more often than the global route's one read per key would.
constexpr u32 HLL_LDS_MAX_LOG2_REGS = 14;
constexpr u32 HLL_LDS_BYTES = 1u << HLL_LDS_MAX_LOG2_REGS;
constexpr u32 HLL_LDS_KEYS_PER_DWORD = 1;
constexpr u32 HLL_BINS = 64;        // bins of one array: a register holds 0 .. 65 - p <= 61
constexpr u32 HLL_STATS_IPT = 4;    // uint4 pieces per thread and grid step of the stats

// bytewise max of four registers: the even and the odd bytes in 16-bit fields; bit 8 of (a | 0x100) - b says a >= b
__device__ __forceinline__ u32 max4(u32 a, u32 b) {
    const u32 ae = a & 0x00FF00FFu, be = b & 0x00FF00FFu, ao = (a >> 8) & 0x00FF00FFu, bo = (b >> 8) & 0x00FF00FFu;
    const u32 ge = (((ae | 0x01000100u) - be) >> 8) & 0x00010001u, go = (((ao | 0x01000100u) - bo) >> 8) & 0x00010001u;
    const u32 me = ge * 0xFFu, mo = go * 0xFFu;   // 0x00FF per field where a >= b
    return ((ae & me) | (be & ~me)) | (((ao & mo) | (bo & ~mo)) << 8);
}

// register and rank of a hash (kmx.h, UPDATE): the sentinel bit below the rank's bits makes w == 0 count 64 - p zeros
__device__ __forceinline__ void reg_rank(u64 h, u32 p, u32* idx, u32* rank) {
    *idx = (u32)(h >> (64u - p));
    *rank = (u32)__clzll((long long)((h << p) | (1ull << (p - 1u)))) + 1u;
}

// max(register, rank) into one byte of an aligned dword, the other three carried unchanged.  SCOPE: workgroup for the LDS array,
// agent for the caller's.
template <int SCOPE>
__device__ __forceinline__ void reg_raise(u32* word, u32 byte, u32 rank) {
    const u32 sh = 8u * byte;
    u32 old = __hip_atomic_load(word, __ATOMIC_RELAXED, SCOPE);
    for (;;) {
        if (((old >> sh) & 255u) >= rank) return;
        const u32 want = (old & ~(255u << sh)) | (rank << sh);
        if (__hip_atomic_compare_exchange_strong(word, &old, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE)) return;
    }
}

// flags == nullptr: every key counts, otherwise those with KMX_WIN_VALID.  PRIV: the block-private route (p <= HLL_LDS_MAX_LOG2_REGS).
template <u32 W, bool PRIV>
__global__ void __launch_bounds__(CT) hll_add_kernel(const u64* __restrict__ keys, const uint8_t* __restrict__ flags, u64 n, uint8_t* regs, u32 p,
                                                     u64 seed) {
    const u64 stride = (u64)gridDim.x * CT;
    u32* const g = reinterpret_cast<u32*>(regs);
    if constexpr (PRIV) {
        __shared__ u32 priv[HLL_LDS_BYTES / 4u];
        const u32 n_dw = (1u << p) >> 2;   // (p >= 4: at least four dwords)
        for (u32 d = threadIdx.x; d < n_dw; d += CT) priv[d] = 0u;
        __syncthreads();
        for (u64 i = (u64)blockIdx.x * CT + threadIdx.x; i < n; i += stride) {
            if (flags != nullptr && (flags[i] & KMX_WIN_VALID) == 0u) continue;
            u32 idx, rank;
            reg_rank(key_hash<W>(Key<W>::load(keys, i), seed), p, &idx, &rank);
            reg_raise<__HIP_MEMORY_SCOPE_WORKGROUP>(&priv[idx >> 2], idx & 3u, rank);
        }
        __syncthreads();
        for (u32 d = threadIdx.x; d < n_dw; d += CT) {
            const u32 mine = priv[d];
            if (mine == 0u) continue;
            u32 old = __hip_atomic_load(&g[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (;;) {
                const u32 want = max4(old, mine);
                if (want == old) break;
                if (__hip_atomic_compare_exchange_strong(&g[d], &old, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
            }
        }
    } else {
        for (u64 i = (u64)blockIdx.x * CT + threadIdx.x; i < n; i += stride) {
            if (flags != nullptr && (flags[i] & KMX_WIN_VALID) == 0u) continue;
            u32 idx, rank;
            reg_rank(key_hash<W>(Key<W>::load(keys, i), seed), p, &idx, &rank);
            reg_raise<__HIP_MEMORY_SCOPE_AGENT>(&g[idx >> 2], idx & 3u, rank);
        }
    }
}

// (no __restrict__: out may be a or b)
__global__ void __launch_bounds__(CT) hll_merge_kernel(const uint4* a, const uint4* b, u64 n16, uint4* out) {
    const u64 stride = (u64)gridDim.x * CT;
    for (u64 i = (u64)blockIdx.x * CT + threadIdx.x; i < n16; i += stride) {
        const uint4 x = a[i], y = b[i];
        out[i] = make_uint4(max4(x.x, y.x), max4(x.y, y.y), max4(x.z, y.z), max4(x.w, y.w));
    }
}

// the number of zero bytes of a dword
__device__ __forceinline__ u32 zero_bytes(u32 v) {
    const u32 nz = ((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v;   // bit 7 of a byte: the byte is not zero
    return 4u - (u32)__popc(nz & 0x80808080u);
}

// the non-zero bytes of a dword into the 64 LDS bins at `bins` (a byte above 63, which no call writes, lands in bin 63); returns
// the number of zero bytes
__device__ __forceinline__ u32 tally4(u32 v, u32* bins) {
    const u32 z = zero_bytes(v);
    if (z != 4u) {
#pragma unroll
        for (u32 s = 0; s < 32u; s += 8u) {
            const u32 c = (v >> s) & 255u;
            if (c) atomicAdd(&bins[c < HLL_BINS ? c : HLL_BINS - 1u], 1u);
        }
    }
    return z;
}

// b == nullptr: the 64 bins of a; otherwise 192: those of a, of b and of max(a, b)
__global__ void __launch_bounds__(CT) hll_stats_kernel(const uint4* __restrict__ a, const uint4* __restrict__ b, u64 n16, u64 per_block,
                                                       unsigned long long* hist) {
    __shared__ u32 bins[3u * HLL_BINS];
    if (threadIdx.x < 3u * HLL_BINS) bins[threadIdx.x] = 0u;
    __syncthreads();
    const u64 lo = (u64)blockIdx.x * per_block, hi = lo + per_block < n16 ? lo + per_block : n16;
    u64 za = 0, zb = 0, zm = 0;
    for (u64 i = lo + threadIdx.x; i < hi; i += CT) {
        const uint4 v = a[i];
        const u32 x[4] = {v.x, v.y, v.z, v.w};
        if (b == nullptr) {
#pragma unroll
            for (u32 q = 0; q < 4; ++q) za += tally4(x[q], bins);
        } else {
            const uint4 u = b[i];
            const u32 y[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (u32 q = 0; q < 4; ++q) {
                za += tally4(x[q], bins);
                zb += tally4(y[q], bins + HLL_BINS);
                zm += tally4(max4(x[q], y[q]), bins + 2u * HLL_BINS);
            }
        }
    }
    za = wave_sum_shfl(za);
    zb = wave_sum_shfl(zb);
    zm = wave_sum_shfl(zm);
    if ((threadIdx.x & 63u) == 0u) {
        if (za) atomicAdd(&hist[0], (unsigned long long)za);
        if (zb) atomicAdd(&hist[HLL_BINS], (unsigned long long)zb);
        if (zm) atomicAdd(&hist[2u * HLL_BINS], (unsigned long long)zm);
    }
    __syncthreads();
    if (threadIdx.x < (b == nullptr ? HLL_BINS : 3u * HLL_BINS)) {
        const u32 c = bins[threadIdx.x];
        if (c) atomicAdd(&hist[threadIdx.x], (unsigned long long)c);
    }
}
static_assert(3u * HLL_BINS <= CT, "the stats kernel keeps at most one bin per thread");

// the route of an add of n keys: block-private where the array fits the LDS cut and every block has a key per dword it flushes
bool hll_add_block_private(u64 n, u32 log2_regs, int n_cu) {
    if (log2_regs > HLL_LDS_MAX_LOG2_REGS) return false;
    const u64 flushed = (1ull << log2_regs) >> 2;   // dwords a block flushes
    return n >= (u64)sweep_blocks(n, n_cu) * flushed * HLL_LDS_KEYS_PER_DWORD;
}

}  // namespace

// ---------------------------------------------------------------- host side

hipError_t launch_hll_add(u32 words, const u64* keys, const uint8_t* flags, u64 n, uint8_t* regs, u32 log2_regs, u64 seed, int n_cu, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const bool priv = hll_add_block_private(n, log2_regs, n_cu);
    with_width(words, [&](auto w) {
        constexpr u32 W = decltype(w)::value;
        if (priv)
            hipLaunchKernelGGL((hll_add_kernel<W, true>), dim3(sweep_blocks(n, n_cu)), dim3(CT), 0, st, keys, flags, n, regs, log2_regs, seed);
        else
            hipLaunchKernelGGL((hll_add_kernel<W, false>), dim3(sweep_blocks(n, n_cu)), dim3(CT), 0, st, keys, flags, n, regs, log2_regs, seed);
    });
    return hipGetLastError();
}

hipError_t launch_hll_merge(const uint8_t* a, const uint8_t* b, u32 log2_regs, uint8_t* out, int n_cu, hipStream_t st) {
    const u64 n16 = (1ull << log2_regs) >> 4;
    hipLaunchKernelGGL(hll_merge_kernel, dim3(sweep_blocks(n16, n_cu)), dim3(CT), 0, st, reinterpret_cast<const uint4*>(a),
                       reinterpret_cast<const uint4*>(b), n16, reinterpret_cast<uint4*>(out));
    return hipGetLastError();
}

hipError_t launch_hll_stats(const uint8_t* a, const uint8_t* b, u32 log2_regs, u64* hist, int n_cu, hipStream_t st) {
    const u64 n16 = (1ull << log2_regs) >> 4;
    // a block's share: whole steps of the block (2^24 registers at the most: its LDS bins cannot wrap)
    u64 nb = ceil_div(n16, (u64)CT * HLL_STATS_IPT);
    const u64 cap = (u64)(n_cu > 0 ? n_cu : 256) * 8u;
    if (nb > cap) nb = cap;
    const u64 per_block = ceil_div(ceil_div(n16, nb), CT) * CT;
    nb = ceil_div(n16, per_block);
    hipLaunchKernelGGL(hll_stats_kernel, dim3((unsigned)nb), dim3(CT), 0, st, reinterpret_cast<const uint4*>(a), reinterpret_cast<const uint4*>(b),
                       n16, per_block, reinterpret_cast<unsigned long long*>(hist));
    return hipGetLastError();
}

}  // namespace kmx
