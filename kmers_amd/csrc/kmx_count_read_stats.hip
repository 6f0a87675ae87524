// kmx_count_read_stats.hip -- per-read abundance statistics against a count table (kmx_count_read_stats(2)): a segmented reduction
// over what kmx_count_lookup_reads(2) leaves -- one u64 count and one flag byte per window -- into KMX_RS_WORDS u64 per read.  The
// segments are the reads: r * W windows apart (uniform reads) or between win_offsets[r] and win_offsets[r + 1] (ragged reads; the
// offsets are made on the device by launch_count_win_offsets).  Key width plays no part here: counts are u64 for either.
//
// One read, three sizes:
//   short   at most 64 * NC windows, NC = 1, 2 or 4 (256 windows: every short-read workload).  One wave per read, window p of the
//           read in lane p % 64, register p / 64.  Counts of windows are wave ballots, min / max / sum and the span are DPP
//           reductions (kmx_device.h); no LDS, no atomics.
//   long    up to BLOCK_MIN windows: one wave per read, 64 windows per step; the select re-streams counts and flags per bit.
//   block   above BLOCK_MIN windows: the same code with a block of 256 lanes as the group (four ballots per step and the
//           reductions go through LDS).  Asked to be exact, not fast.
// Uniform batches pick one kernel on the host.  Ragged batches run the short kernel, which skips what it cannot hold, and then one
// pass over the window offsets (64 reads per step of a block, every wave of the block loading the same 64 so that no LDS is needed
// to agree on them) that hands the long reads to the block's waves in turn and the block-sized ones to the whole block.  No
// block waits for another; every row is written by exactly one wave or block, so repeated calls are bit-identical.
//
// Median.  c[n_valid / 2] of the valid windows' counts in ascending unsigned order, by most-significant-bit-first radix select: min
// and max come out of the first pass; all values share the bits above the highest bit in which min and max differ, so the select
// walks only the bits from there down (real counts are small: a handful of steps, none when min == max).  Per bit: how many
// candidates have a 0 there (ballots / a group sum), then the rank decides the bit and the candidates narrow.  Exact for any u64.
//
// Span.  "Length of the solid run ending here" for every window: with b = the ballot of `solid` over the 64 windows of a step, a
// lane's run reaches back to the highest 0 bit of b at or below it, or, if there is none, through the whole step into the run the
// previous steps carried.  The answer is the maximum of (length << 32 | ~start) over all windows: length descending, then start
// ascending, whatever order the lanes are reduced in.
#include "kmx_count_common.h"

namespace kmx {

namespace {

constexpr u32 RS_BLOCK_MIN = 8192;   // a read of more windows than this gets a whole block

__device__ __forceinline__ u64 max64(u64 a, u64 b) { return a > b ? a : b; }

// max over the 64 lanes of a 64-bit value, wave-uniform: DPP inside the rows of 16 lanes, the four rows through v_readlane
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
    v = max64(v, KMX_DPP64(v, 0xB1 /* quad_perm:[1,0,3,2] */));
    v = max64(v, KMX_DPP64(v, 0x4E /* quad_perm:[2,3,0,1] */));
    v = max64(v, KMX_DPP64(v, 0x124 /* row_ror:4 */));
    v = max64(v, KMX_DPP64(v, 0x128 /* row_ror:8 */));
    const u32 lo = (u32)v, hi = (u32)(v >> 32);
    u64 r = 0;
#pragma unroll
    for (int l = 0; l < 64; l += 16)
        r = max64(r, ((u64)(u32)__builtin_amdgcn_readlane((int)hi, l) << 32) | (u32)__builtin_amdgcn_readlane((int)lo, l));
    return r;
}
__device__ __forceinline__ u64 wave_min_u64(u64 v) { return ~wave_max_u64(~v); }

__device__ __forceinline__ u32 clz64(u64 v) { return (u32)__clzll((long long)v); }   // (v != 0)

// bits 0 .. lane of a 64-bit mask
__device__ __forceinline__ u64 upto(u32 lane) { return lane == 63u ? ~0ull : (2ull << lane) - 1ull; }

// the solid run that ends at the last window of a step whose ballot is b, given the run carried into the step
__device__ __forceinline__ u32 carry_through(u64 b, u32 carry) { return b == ~0ull ? carry + 64u : clz64(~b); }

// (length, start) of a run as one word to maximise: longer first, then earlier
__device__ __forceinline__ u64 span_key(u32 len, u32 start) { return ((u64)len << 32) | (u64)(0xFFFFFFFFu - start); }
__device__ __forceinline__ u64 span_word(u64 key) { return key == 0u ? 0u : (key & 0xFFFFFFFF00000000ull) | (u64)(0xFFFFFFFFu - (u32)key); }

struct Row {
    u64 n_valid, n_present, n_solid, mn, mx, sum, median, span;
};
// lanes 0 .. 7 of a group write the row's words: one 64-byte store
__device__ __forceinline__ void write_row(u64* __restrict__ row, u32 t, const Row& s) {
    if (t >= KMX_RS_WORDS) return;
    const u64 v = t == KMX_RS_N_VALID ? s.n_valid : t == KMX_RS_N_PRESENT ? s.n_present : t == KMX_RS_N_SOLID ? s.n_solid
                : t == KMX_RS_MIN ? s.mn : t == KMX_RS_MAX ? s.mx : t == KMX_RS_SUM ? s.sum : t == KMX_RS_MEDIAN ? s.median : s.span;
    row[t] = v;
}

// ---------------------------------------------------------------- short reads: one wave, counts in registers
template <u32 NC, bool RAGGED>
__global__ void __launch_bounds__(CT) read_stats_short_kernel(const u64* __restrict__ counts, const uint8_t* __restrict__ flags,
                                                              const u64* __restrict__ wo, u64 n_reads, u32 W, u64 solid_min,
                                                              u64* __restrict__ stats) {
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 stride = (u64)gridDim.x * (CT / 64u);
    for (u64 r = (u64)blockIdx.x * (CT / 64u) + wave; r < n_reads; r += stride) {
        u64 w0;
        u32 nwin;
        if (RAGGED) {
            w0 = wo[r];
            const u64 d = wo[r + 1u] - w0;
            if (d > 64u * NC) continue;   // (the long pass writes this read's row)
            nwin = (u32)d;
        } else {
            w0 = r * W;
            nwin = W;
        }
        u64 c[NC];
        bool v[NC];
#pragma unroll
        for (u32 j = 0; j < NC; ++j) {
            const u32 p = j * 64u + lane;
            v[j] = p < nwin && (flags[w0 + p] & KMX_WIN_VALID) != 0u;
            c[j] = v[j] ? counts[w0 + p] : 0u;
        }
        u32 nv = 0, np = 0, ns = 0, carry = 0;
        u64 mx = 0, mn = ~0ull, sum = 0, best = 0;
#pragma unroll
        for (u32 j = 0; j < NC; ++j) {
            const bool solid = v[j] && c[j] >= solid_min;
            const u64 bs = __ballot(solid);
            nv += (u32)__popcll(__ballot(v[j]));
            np += (u32)__popcll(__ballot(v[j] && c[j] != 0u));
            ns += (u32)__popcll(bs);
            if (v[j]) {
                mx = max64(mx, c[j]);
                mn = c[j] < mn ? c[j] : mn;
                sum += c[j];
            }
            if (solid) {
                const u64 z = ~bs & upto(lane);   // the windows of this step, at or below this one, that are not solid
                const u32 run = z ? lane - (63u - clz64(z)) : lane + 1u + carry;
                best = max64(best, span_key(run, j * 64u + lane + 1u - run));
            }
            carry = carry_through(bs, carry);
        }
        Row s;
        s.n_valid = nv;
        s.n_present = np;
        s.n_solid = ns;
        s.mx = wave_max_u64(mx);
        s.mn = nv ? wave_min_u64(mn) : 0u;
        s.sum = wave_sum(sum);
        s.span = span_word(wave_max_u64(best));
        s.median = s.mx;   // (min == max, or no valid window: 0)
        if (s.mx != s.mn) {
            u32 t = nv / 2u;
            const u32 top = 63u - clz64(s.mx ^ s.mn);
            u64 prefix = top == 63u ? 0u : (s.mx >> (top + 1u)) << (top + 1u);
            bool cand[NC];
#pragma unroll
            for (u32 j = 0; j < NC; ++j) cand[j] = v[j];
            for (int b = (int)top; b >= 0; --b) {
                u32 zeros = 0;
#pragma unroll
                for (u32 j = 0; j < NC; ++j) zeros += (u32)__popcll(__ballot(cand[j] && ((c[j] >> b) & 1ull) == 0u));
                const bool one = t >= zeros;
                if (one) {
                    t -= zeros;
                    prefix |= 1ull << b;
                }
#pragma unroll
                for (u32 j = 0; j < NC; ++j) cand[j] = cand[j] && (((c[j] >> b) & 1ull) != 0u) == one;
            }
            s.median = prefix;
        }
        write_row(stats + KMX_RS_WORDS * r, lane, s);
    }
}

// ---------------------------------------------------------------- long reads: a group (a wave, or the block) streams the read
// what a group of lanes agrees on; `sh` holds 8 u64 (BLOCK only: [0, 4) the waves' ballots, [4, 8) their partial results)
template <bool BLOCK, typename Op>
__device__ __forceinline__ u64 group_combine(u64 wave_value, u64* sh, Op op) {
    if (!BLOCK) return wave_value;
    if ((threadIdx.x & 63u) == 0u) sh[4u + (threadIdx.x >> 6)] = wave_value;
    __syncthreads();
    const u64 r = op(op(sh[4], sh[5]), op(sh[6], sh[7]));
    __syncthreads();
    return r;
}
template <bool BLOCK> __device__ __forceinline__ u64 group_sum(u64 v, u64* sh) {
    return group_combine<BLOCK>(wave_sum(v), sh, [](u64 a, u64 b) { return a + b; });
}
template <bool BLOCK> __device__ __forceinline__ u64 group_max(u64 v, u64* sh) {
    return group_combine<BLOCK>(wave_max_u64(v), sh, [](u64 a, u64 b) { return max64(a, b); });
}

// Every lane of the group calls this with the same arguments (the group is at a uniform point, BLOCK: the whole block).
template <bool BLOCK>
__device__ __forceinline__ void long_read_stats(const u64* __restrict__ counts, const uint8_t* __restrict__ flags, u64 w0, u32 nwin,
                                                u64 solid_min, u64* __restrict__ row, u64* sh) {
    constexpr u32 G = BLOCK ? CT : 64u, NW = G / 64u;
    const u32 lane = threadIdx.x & 63u, wi = BLOCK ? threadIdx.x >> 6 : 0u, t = wi * 64u + lane;
    u64 nv = 0, np = 0, ns = 0, mx = 0, mn = ~0ull, sum = 0, best = 0;
    u32 carry = 0;   // the solid run that ends at the last window of the previous step
    for (u32 base = 0; base < nwin; base += G) {   // (nwin < 2^31: base + G does not wrap)
        const u32 p = base + t;
        const bool valid = p < nwin && (flags[w0 + p] & KMX_WIN_VALID) != 0u;
        const u64 c = valid ? counts[w0 + p] : 0u;
        const bool solid = valid && c >= solid_min;
        if (valid) {
            ++nv;
            np += c != 0u;
            ns += solid;
            mx = max64(mx, c);
            mn = c < mn ? c : mn;
            sum += c;
        }
        const u64 mine = __ballot(solid);
        u64 m[NW];
        if (BLOCK) {
            if (lane == 0u) sh[wi] = mine;
            __syncthreads();
#pragma unroll
            for (u32 w = 0; w < NW; ++w) m[w] = sh[w];
            __syncthreads();
        } else {
            m[0] = mine;
        }
        if (solid) {
            const u64 z = ~mine & upto(lane);
            u32 run;
            if (z) {
                run = lane - (63u - clz64(z));
            } else {   // through the waves below this one, as far as they are all solid, then into the carried run
                run = lane + 1u;
                bool open = true;
#pragma unroll
                for (int w = (int)NW - 2; w >= 0; --w) {
                    if (open && (u32)w < wi) {
                        if (m[w] == ~0ull) run += 64u;
                        else {
                            run += clz64(~m[w]);
                            open = false;
                        }
                    }
                }
                if (open) run += carry;
            }
            best = max64(best, span_key(run, p + 1u - run));
        }
#pragma unroll
        for (u32 w = 0; w < NW; ++w) carry = carry_through(m[w], carry);
    }
    Row s;
    s.n_valid = group_sum<BLOCK>(nv, sh);
    s.n_present = group_sum<BLOCK>(np, sh);
    s.n_solid = group_sum<BLOCK>(ns, sh);
    s.mx = group_max<BLOCK>(mx, sh);
    s.mn = s.n_valid ? ~group_max<BLOCK>(~mn, sh) : 0u;
    s.sum = group_sum<BLOCK>(sum, sh);
    s.span = span_word(group_max<BLOCK>(best, sh));
    s.median = s.mx;
    if (s.mx != s.mn) {
        u64 rank = s.n_valid / 2u;
        const u32 top = 63u - clz64(s.mx ^ s.mn);
        u64 prefix = top == 63u ? 0u : (s.mx >> (top + 1u)) << (top + 1u);
        for (int b = (int)top; b >= 0; --b) {
            const u64 above = b == 63 ? 0u : ~0ull << (b + 1);   // the bits already decided
            u64 zeros = 0;
            for (u32 base = 0; base < nwin; base += G) {
                const u32 p = base + t;
                if (p < nwin && (flags[w0 + p] & KMX_WIN_VALID) != 0u) {
                    const u64 c = counts[w0 + p];
                    zeros += (c & above) == prefix && ((c >> b) & 1ull) == 0u;
                }
            }
            zeros = group_sum<BLOCK>(zeros, sh);
            if (rank >= zeros) {
                rank -= zeros;
                prefix |= 1ull << b;
            }
        }
        s.median = prefix;
    }
    write_row(row, t, s);
}

// uniform reads of more than 256 windows: a wave (BLOCK: the block) per read
template <bool BLOCK>
__global__ void __launch_bounds__(CT) read_stats_long_uniform_kernel(const u64* __restrict__ counts, const uint8_t* __restrict__ flags, u64 n_reads,
                                                                     u32 W, u64 solid_min, u64* __restrict__ stats) {
    __shared__ u64 sh[8];
    const u32 per = BLOCK ? 1u : CT / 64u;
    const u32 wave = BLOCK ? 0u : (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (u64 r = (u64)blockIdx.x * per + wave; r < n_reads; r += (u64)gridDim.x * per)
        long_read_stats<BLOCK>(counts, flags, r * W, W, solid_min, stats + KMX_RS_WORDS * r, sh);
}

// ragged reads the short kernel skipped (more than short_max windows).  A block looks at 64 reads per step -- each of its waves loads
// the same 64 window offsets, so all four hold the same two ballots -- and takes the long reads wave by wave, in turn, and then the
// block-sized ones together.
__global__ void __launch_bounds__(CT) read_stats_long_ragged_kernel(const u64* __restrict__ counts, const uint8_t* __restrict__ flags,
                                                                    const u64* __restrict__ wo, u64 n_reads, u32 short_max, u64 solid_min,
                                                                    u64* __restrict__ stats) {
    __shared__ u64 sh[8];
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (u64 r0 = (u64)blockIdx.x * 64u; r0 < n_reads; r0 += (u64)gridDim.x * 64u) {
        u64 d = 0;
        if (r0 + lane < n_reads) d = wo[r0 + lane + 1u] - wo[r0 + lane];
        u64 by_wave = __ballot(d > short_max && d <= RS_BLOCK_MIN);
        u64 by_block = __ballot(d > RS_BLOCK_MIN);
        for (u32 i = 0; by_wave; ++i) {
            const u64 r = r0 + (u64)(__ffsll((long long)by_wave) - 1);
            by_wave &= by_wave - 1ull;
            if ((i & 3u) != wave) continue;
            const u64 w0 = wo[r];
            long_read_stats<false>(counts, flags, w0, (u32)(wo[r + 1u] - w0), solid_min, stats + KMX_RS_WORDS * r, sh);
        }
        while (by_block) {   // (the same mask in every wave: the whole block walks it together)
            const u64 r = r0 + (u64)(__ffsll((long long)by_block) - 1);
            by_block &= by_block - 1ull;
            const u64 w0 = wo[r];
            long_read_stats<true>(counts, flags, w0, (u32)(wo[r + 1u] - w0), solid_min, stats + KMX_RS_WORDS * r, sh);
        }
    }
}

unsigned grid_for(u64 units, int n_cu, u32 per_cu) {
    const u64 cap = (u64)(n_cu > 0 ? n_cu : 256) * per_cu;
    return (unsigned)(units < cap ? (units ? units : 1u) : cap);
}

template <bool RAGGED>
void launch_short(u32 w_max, const u64* counts, const uint8_t* flags, const u64* wo, u64 n_reads, u32 W, u64 solid_min, u64* stats, int n_cu,
                  hipStream_t st) {
    const dim3 g(grid_for(ceil_div(n_reads, CT / 64u), n_cu, 64u)), b(CT);
    if (w_max <= 64u) hipLaunchKernelGGL((read_stats_short_kernel<1, RAGGED>), g, b, 0, st, counts, flags, wo, n_reads, W, solid_min, stats);
    else if (w_max <= 128u) hipLaunchKernelGGL((read_stats_short_kernel<2, RAGGED>), g, b, 0, st, counts, flags, wo, n_reads, W, solid_min, stats);
    else hipLaunchKernelGGL((read_stats_short_kernel<4, RAGGED>), g, b, 0, st, counts, flags, wo, n_reads, W, solid_min, stats);
}

}  // namespace

// counts / flags: one u64 and one byte per window, as launch_count_lookup leaves them.  win_offsets == nullptr: uniform reads of W
// windows each (W >= 1).  Otherwise ragged reads, n_reads + 1 device offsets; W = the most windows a read is expected to have (a
// hint that picks the short kernel's frame: 0 = unknown; a read above it is served all the same).  stats: KMX_RS_WORDS u64 per read.
hipError_t launch_count_read_stats(const u64* counts, const uint8_t* flags, const u64* win_offsets, u64 n_reads, u32 W, u64 solid_min, u64* stats,
                                   int n_cu, hipStream_t st) {
    if (n_reads == 0) return hipSuccess;
    if (!win_offsets) {
        if (W <= 256u) {
            launch_short<false>(W, counts, flags, nullptr, n_reads, W, solid_min, stats, n_cu, st);
        } else if (W <= RS_BLOCK_MIN) {
            hipLaunchKernelGGL(read_stats_long_uniform_kernel<false>, dim3(grid_for(ceil_div(n_reads, CT / 64u), n_cu, 64u)), dim3(CT), 0, st, counts,
                               flags, n_reads, W, solid_min, stats);
        } else {
            hipLaunchKernelGGL(read_stats_long_uniform_kernel<true>, dim3(grid_for(n_reads, n_cu, 64u)), dim3(CT), 0, st, counts, flags, n_reads, W,
                               solid_min, stats);
        }
        return hipGetLastError();
    }
    const u32 w_max = W == 0u || W > 256u ? 256u : W;
    const u32 short_max = w_max <= 64u ? 64u : w_max <= 128u ? 128u : 256u;
    launch_short<true>(w_max, counts, flags, win_offsets, n_reads, 0u, solid_min, stats, n_cu, st);
    hipLaunchKernelGGL(read_stats_long_ragged_kernel, dim3(grid_for(ceil_div(n_reads, 64u), n_cu, 64u)), dim3(CT), 0, st, counts, flags, win_offsets,
                       n_reads, short_max, solid_min, stats);
    return hipGetLastError();
}

}  // namespace kmx
