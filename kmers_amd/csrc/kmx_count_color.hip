// kmx_count_color.hip -- the two reductions over a COLOURED table (include/kmx.h: a table whose u64 per key is a bit mask of the
// samples, "colours", at most 64, that hold the key): kmx_count_color_matrix and kmx_count_read_colors(2).  Only the low n_colors
// bits of a mask count, everywhere here: the MASKED mask.  Key width plays no part: both kernels read u64 masks only.
//
// color_matrix_kernel<CB>.  CB = the colour bound, n_colors rounded up to 8 / 16 / 32 / 64 on the host, so that a lane's CB
// accumulators are statically indexed registers.  A wave takes 64 masks per step, grid-stride.  One ballot per colour transposes the
// 64 x 64 bit tile: lane i keeps the ballot of "bit i set" over the step's 64 keys, column i.  Then for every j below CB the wave
// reads column j out of lane j (v_readlane) and lane i adds popcount(col_i & col_j) to acc[j]: after the last step acc[j] of lane i
// is matrix[i][j] of the wave's keys.  The spectrum is the popcount of the lane's own mask, counted into 65 bins of LDS.
//   32-bit accumulators cannot wrap: a step adds at most 64 to one; the launcher caps the grid at CM_MIN_CAP blocks or more and gives
//   every step below the cap a wave of its own, so a wave takes at most ceil(2^34 / (4 * CM_MIN_CAP)) = 2^23 steps of the 2^34 the
//   call accepts (n <= 2^40): below 2^29 per wave, below 2^31 for the four waves of a block folded in LDS (u32 as well).
//   The fold: LDS atomics of the four waves into one CB x 64 tile, then the block writes ITS partial matrix and spectrum into the work
//   buffer, and color_sum_kernel adds the partials up in a fixed order and OVERWRITES the outputs.  No global atomics, no zeroing of
//   the outputs, and the sum of integers is the same whatever the blocks' timing: bit-identical between calls.
//
// read_colors_kernel.  One wave per read, steps of 64 window positions, reads of any length through the same loop (the shape of
// correct_kernel), waves striding over the reads.  Lane = window position within a step for the masks; lane = colour for the hit
// counts: one ballot per colour and step gives colour c's windows, and lane c adds its popcount.  ALL / ANY are DPP reductions of the
// lanes' running AND / OR; N_SWITCH compares every window with its lower neighbour, lane 0 with the last window of the step before.
// No LDS, no atomics, no scratch; a row and its hit counts have one writer, so repeated calls are bit-identical.
#include "kmx_count_common.h"

namespace kmx {

namespace {

constexpr u32 CM_BLOCKS_PER_CU = 4;   // the matrix grid's cap: VALU-bound, four waves per SIMD keep it busy and the partials few
constexpr u32 CM_MIN_CAP = 512;       // ... and never below this many blocks (the bound of the 32-bit accumulators, above)
constexpr u32 CM_SPEC = 65;           // spectrum bins: 0 .. 64 colours
constexpr u32 RC_BLOCKS_PER_CU = 16;  // the read kernel's cap: a wave takes the reads of its index modulo the grid's waves

__host__ __device__ __forceinline__ u64 color_mask(u32 n_colors) { return n_colors >= 64u ? ~0ull : (1ull << n_colors) - 1ull; }
__host__ __device__ __forceinline__ u32 color_bound(u32 n_colors) { return n_colors <= 8u ? 8u : n_colors <= 16u ? 16u : n_colors <= 32u ? 32u : 64u; }
// u64 per block of partials: the CB x CB matrix (index j * CB + i) and the spectrum
__host__ __device__ __forceinline__ u64 partial_words(u32 cb) { return (u64)cb * cb + CM_SPEC; }

__device__ __forceinline__ u64 readlane64(u64 v, u32 l) {
    return ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), (int)l) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)v, (int)l);
}

// Lane i of (lo, hi), for i = I .. CB - 1: the ballot of "bit i of m set" -- column i of the wave's 64 x 64 bit tile.  v_writelane with the
// lane as an immediate, not a select on lane == i: CB loop-invariant lane predicates would be hoisted into scalar register pairs,
// more than there are.  The compiler has no builtin for the instruction and does not look into inline assembly for hazards, so the
// wait states gfx950 asks for are spelled out: two between a VALU instruction that writes a scalar register (the compare behind the
// ballot) and a VALU instruction that reads it -- the s_nop 1 in front --, and one between a VALU write of a vector register and a
// v_readlane of it -- columns_done, behind the last v_writelane.
template <u32 I, u32 CB>
__device__ __forceinline__ void columns_from(u64 m, u32& lo, u32& hi) {
    if constexpr (I < CB) {
        if (I % 8u == 0u) __builtin_amdgcn_sched_barrier(0);   // (eight ballots in flight, not CB: they live in scalar register pairs too)
        const u64 b = __ballot(((m >> I) & 1ull) != 0u);
        asm("s_nop 1\n\tv_writelane_b32 %0, %2, %4\n\tv_writelane_b32 %1, %3, %4" : "+v"(lo), "+v"(hi) : "s"((u32)b), "s"((u32)(b >> 32)), "n"(I));
        columns_from<I + 1u, CB>(m, lo, hi);
    }
}
__device__ __forceinline__ void columns_done(u32& lo, u32& hi) { asm("s_nop 0" : "+v"(lo), "+v"(hi)); }

// AND / OR / max over the 64 lanes of a 64-bit value, wave-uniform: DPP inside the rows of 16 lanes (every lane of these patterns has a
// source lane), the four rows through v_readlane
template <typename Op>
__device__ __forceinline__ u64 wave_fold_u64(u64 v, Op op) {
    v = op(v, KMX_DPP64(v, 0xB1 /* quad_perm:[1,0,3,2] */));
    v = op(v, KMX_DPP64(v, 0x4E /* quad_perm:[2,3,0,1] */));
    v = op(v, KMX_DPP64(v, 0x124 /* row_ror:4 */));
    v = op(v, KMX_DPP64(v, 0x128 /* row_ror:8 */));
    return op(op(readlane64(v, 0u), readlane64(v, 16u)), op(readlane64(v, 32u), readlane64(v, 48u)));
}

// ---------------------------------------------------------------- the pairwise matrix and the spectrum
template <u32 CB>
__global__ void __launch_bounds__(CT) color_matrix_kernel(const u64* __restrict__ colors, u64 n, u64 cmask, bool want_spectrum, u64* __restrict__ partial) {
    __shared__ u32 tile[CB * 64u];   // [j][lane]
    __shared__ u32 spec[CM_SPEC];
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (u32 t = threadIdx.x; t < CB * 64u; t += CT) tile[t] = 0u;
    if (threadIdx.x < CM_SPEC) spec[threadIdx.x] = 0u;
    __syncthreads();
    u32 acc[CB];
#pragma unroll
    for (u32 j = 0; j < CB; ++j) acc[j] = 0u;
    const u64 stride = (u64)gridDim.x * CT;
    for (u64 base = ((u64)blockIdx.x * (CT / 64u) + wave) * 64u; base < n; base += stride) {
        const u64 idx = base + lane;
        const bool in = idx < n;
        const u64 m = in ? colors[idx] & cmask : 0u;
        if (want_spectrum && in) atomicAdd(&spec[__popcll(m)], 1u);
        u32 col_lo = 0, col_hi = 0;   // lane i: the keys of this step that have colour i
        columns_from<0u, CB>(m, col_lo, col_hi);
        columns_done(col_lo, col_hi);
        const u64 col = ((u64)col_hi << 32) | col_lo;
#pragma unroll
        for (u32 j = 0; j < CB; ++j) {
            if (j % 8u == 0u) __builtin_amdgcn_sched_barrier(0);   // (the same for the columns read back)
            acc[j] += (u32)__popcll(col & readlane64(col, j));
        }
    }
#pragma unroll
    for (u32 j = 0; j < CB; ++j) atomicAdd(&tile[j * 64u + lane], acc[j]);
    __syncthreads();
    u64* __restrict__ mine = partial + (u64)blockIdx.x * partial_words(CB);
    for (u32 t = threadIdx.x; t < CB * CB; t += CT) mine[t] = tile[(t / CB) * 64u + (t % CB)];
    if (threadIdx.x < CM_SPEC) mine[CB * CB + threadIdx.x] = spec[threadIdx.x];
}

// Element e of the outputs -- e < n_colors^2: matrix[e / n_colors][e % n_colors]; then the n_colors + 1 bins of the spectrum -- summed
// over the n_parts partials: 64 elements per block, its four waves a quarter of the partials each, in a fixed order.
__global__ void __launch_bounds__(CT) color_sum_kernel(const u64* __restrict__ partial, u64 n_parts, u32 cb, u32 n_colors, u64* __restrict__ matrix,
                                                       u64* __restrict__ spectrum) {
    __shared__ u64 sh[CT];
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u32 nm = n_colors * n_colors, e = blockIdx.x * 64u + lane;
    const bool live = e < nm + (spectrum != nullptr ? n_colors + 1u : 0u);
    u64 s = 0;
    if (live) {
        const u64 at = e < nm ? (u64)(e % n_colors) * cb + (e / n_colors) : (u64)cb * cb + (e - nm);
        for (u64 b = wave; b < n_parts; b += CT / 64u) s += partial[b * partial_words(cb) + at];
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    if (wave == 0u && live) {
        s = sh[lane] + sh[64u + lane] + sh[128u + lane] + sh[192u + lane];
        if (e < nm) matrix[e] = s;
        else spectrum[e - nm] = s;
    }
}

u64 matrix_blocks(u64 n, int n_cu) {
    u64 cap = (u64)(n_cu > 0 ? n_cu : 256) * CM_BLOCKS_PER_CU;
    if (cap < CM_MIN_CAP) cap = CM_MIN_CAP;
    const u64 nb = ceil_div(n, CT);   // a step of 64 keys per wave
    return nb < cap ? nb : cap;
}

// ---------------------------------------------------------------- per-read colour sets
// answers / flags: one u64 (the key's mask, 0 = absent) and one byte per window, as the lookup leaves them.  wo == nullptr: uniform
// reads of W windows, read r's at r * W; otherwise the windows wo[r] .. wo[r + 1) (a read without a window: a row of zeros).
__global__ void __launch_bounds__(CT) read_colors_kernel(const u64* __restrict__ answers, const uint8_t* __restrict__ flags, const u64* __restrict__ wo,
                                                         u64 n_reads, u32 W, u32 n_colors, u32 thr_num, u32 thr_den, u64* __restrict__ rows,
                                                         u32* __restrict__ hits_out) {
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 stride = (u64)gridDim.x * (CT / 64u);
    const u64 cmask = color_mask(n_colors);
    for (u64 r = (u64)blockIdx.x * (CT / 64u) + wave; r < n_reads; r += stride) {
        u64 w0;
        u32 nwin;
        if (wo != nullptr) {
            w0 = wo[r];
            nwin = (u32)(wo[r + 1u] - w0);   // (below 2^31: a longer read has no window)
        } else {
            w0 = r * W;
            nwin = W;
        }
        u32 nv = 0, nh = 0, nu = 0, nsw = 0;   // wave-uniform counts
        u32 hits = 0;                          // lane c: the hit windows that have colour c
        u64 all = ~0ull, any = 0u;             // per lane, over its hit windows
        u64 carry = 0u;                        // the masked mask of the window before this step's first (0: none, or not a hit)
        for (u32 s = 0; s < nwin; s += 64u) {  // (nwin < 2^31: s + 64 does not wrap)
            const u32 pos = s + lane;
            u64 m = 0u;
            bool v = false;
            if (pos < nwin) {
                v = (flags[w0 + pos] & KMX_WIN_VALID) != 0u;
                if (v) m = answers[w0 + pos] & cmask;
            }
            const bool hit = m != 0u;
            const u64 bh = __ballot(hit);
            nv += (u32)__popcll(__ballot(v));
            nh += (u32)__popcll(bh);
            nu += (u32)__popcll(__ballot(hit && (m & (m - 1ull)) == 0u));
            if (hit) {
                all &= m;
                any |= m;
            }
            // the window below: lane - 1's, lane 0 takes the step before's last (positions behind the read's end hold 0: no pair there)
            u64 below = __shfl_up(m, 1u);
            if (lane == 0u) below = carry;
            nsw += (u32)__popcll(__ballot(hit && below != 0u && below != m));
            carry = readlane64(m, 63u);
            if (bh != 0u) {
                for (u32 c = 0; c < n_colors; ++c) {
                    const u32 cnt = (u32)__popcll(__ballot(((m >> c) & 1ull) != 0u));
                    if (lane == c) hits += cnt;
                }
            }
        }
        const u64 r_all = nh ? wave_fold_u64(all, [](u64 a, u64 b) { return a & b; }) : 0u;
        const u64 r_any = wave_fold_u64(any, [](u64 a, u64 b) { return a | b; });
        // (hits < 2^31 and thr_den, thr_num < 2^32, nv < 2^31: the products fit a u64)
        const u64 r_thr = __ballot(hits > 0u && (u64)hits * thr_den >= (u64)thr_num * nv);
        const u64 top = wave_fold_u64(((u64)hits << 32) | (u64)(63u - lane), [](u64 a, u64 b) { return a > b ? a : b; });
        const u64 r_best = nh ? (top & 0xFFFFFFFF00000000ull) | (u64)(63u - (u32)(top & 63u)) : 0u;
        if (lane < KMX_RC_WORDS) {
            const u64 x = lane == KMX_RC_N_VALID ? nv : lane == KMX_RC_N_HIT ? nh : lane == KMX_RC_N_UNIQUE ? nu : lane == KMX_RC_ALL ? r_all
                        : lane == KMX_RC_ANY ? r_any : lane == KMX_RC_THRESH ? r_thr : lane == KMX_RC_BEST ? r_best : nsw;
            rows[KMX_RC_WORDS * r + lane] = x;
        }
        if (hits_out != nullptr && lane < n_colors) hits_out[(u64)n_colors * r + lane] = hits;
    }
}

}  // namespace

// ---------------------------------------------------------------- host side
size_t count_color_matrix_bytes(u64 n, u32 n_colors, int n_cu) { return (size_t)(matrix_blocks(n, n_cu) * partial_words(color_bound(n_colors)) * 8u); }

// area: count_color_matrix_bytes(n, n_colors, n_cu) bytes (none for n == 0); spectrum may be nullptr
hipError_t launch_count_color_matrix(const u64* colors, u64 n, u32 n_colors, void* area, u64* matrix, u64* spectrum, int n_cu, hipStream_t st) {
    const u64 nb = matrix_blocks(n, n_cu);
    const u32 cb = color_bound(n_colors);
    u64* partial = static_cast<u64*>(area);
    const u64 cmask = color_mask(n_colors);
    const bool ws = spectrum != nullptr;
    if (nb != 0) {
        const dim3 grid((unsigned)nb), block(CT);
        if (cb == 8u) hipLaunchKernelGGL(color_matrix_kernel<8>, grid, block, 0, st, colors, n, cmask, ws, partial);
        else if (cb == 16u) hipLaunchKernelGGL(color_matrix_kernel<16>, grid, block, 0, st, colors, n, cmask, ws, partial);
        else if (cb == 32u) hipLaunchKernelGGL(color_matrix_kernel<32>, grid, block, 0, st, colors, n, cmask, ws, partial);
        else hipLaunchKernelGGL(color_matrix_kernel<64>, grid, block, 0, st, colors, n, cmask, ws, partial);
    }
    const u32 n_out = n_colors * n_colors + (ws ? n_colors + 1u : 0u);
    hipLaunchKernelGGL(color_sum_kernel, dim3((unsigned)ceil_div(n_out, 64u)), dim3(CT), 0, st, partial, nb, cb, n_colors, matrix, spectrum);
    return hipGetLastError();
}

hipError_t launch_count_read_colors(const u64* answers, const uint8_t* flags, const u64* win_offsets, u64 n_reads, u32 W, u32 n_colors, u32 thr_num,
                                    u32 thr_den, u64* rows, u32* hits, int n_cu, hipStream_t st) {
    if (n_reads == 0) return hipSuccess;
    u64 nb = ceil_div(n_reads, CT / 64u);
    const u64 cap = (u64)(n_cu > 0 ? n_cu : 256) * RC_BLOCKS_PER_CU;
    if (nb > cap) nb = cap;
    hipLaunchKernelGGL(read_colors_kernel, dim3((unsigned)nb), dim3(CT), 0, st, answers, flags, win_offsets, n_reads, W, n_colors, thr_num, thr_den, rows,
                       hits);
    return hipGetLastError();
}

}  // namespace kmx
