// kmx_reads_quality.hip -- one pass over the bases and the quality bytes of a batch of reads: kmx_reads_quality.  kmx.h has the
// contract (the masked copy, the eight words of a row, the Mott span); DESIGN 4.6.15 has the reasoning and the figures.
//
// A WAVE PER READ.  A lane owns four consecutive bytes per step, a wave 256: the hot shape (100-250 bases) is one step, a longer read
// walks through the same code 256 bytes at a time with its state carried in wave-uniform registers (exact, not fast: the way
// kmx_count_read_stats treats a long read).  The grid of four bytes is the dword grid of the OUTPUT (d_masked; of d_bases when
// there is none): A = the address of the read's first output byte mod 4, the lane's byte j of step s is base s + 4 lane + j - A.
// So every store of masked bytes is one aligned dword, except the read's first and last dword where they are partial: those go out
// byte by byte, and not one byte outside the read is written.  Bases and qualities are loaded as aligned dwords, two per lane where
// the source's phase differs from the grid's, lined up by a funnel shift; a dword is loaded only if it holds a byte of the read.
// In place (d_masked == d_bases) a lane loads exactly the dword it stores.
//
// Per lane, two walks over its four bytes.  The first: q, LOW, GOOD, the masked byte, and what the lane contributes to the scans --
// the sum of its q - trim_q, the last position that is not GOOD, its sums.  Between them three DPP scans over the wave (row_shr
// inside the rows of 16, then the two row broadcasts): a max-scan of "last bad position" (the run that ends at a base is its
// position minus that: carry_through / span_key of kmx_count_read_stats.hip, with the position in place of the window), an add-scan
// of the partial sums P, and a min-scan of the key (P relative to the step, index) whose minimum is the smallest prefix sum and,
// of equal ones, the LAST -- the a* of the Mott span.  P is kept relative to the step's first byte, so the packed key holds for a
// read of any length: the carried minimum (64 bits, absolute) is compared outside the scan.  The second walk: prefix minimum, D =
// P_b - min, the run that ends at each base, the windows.  Then the wave's best D and best run (a max over the lanes, a ballot of
// the lanes that hold it, the lowest of them: the smallest b, the leftmost run) and the sums.
// The weight table (256 u64) is staged in LDS once per block: a lane gathers four words of it per step.
// No atomics, no scratch; a row is written by the eight low lanes of the one wave that owns the read.
// The bounds of a read, "is one of ACGTacgt" and the wave-per-read launch shape are the family's (kmx_reads_common.h).
#include "kmx_reads_common.h"

namespace kmx {

namespace {

constexpr u32 RQ_LANE = 4;                 // bytes a lane owns per step
constexpr u32 RQ_STEP = 64u * RQ_LANE;     // bytes a wave handles per step

// op(earlier, later) over the lanes before and at this one.  `ident`: what a lane without a source gets (update_dpp keeps `old`).
#define KMX_RQ_DPP32(ident, v, ctrl, rows) ((u32)__builtin_amdgcn_update_dpp((int)(ident), (int)(v), (ctrl), (rows), 0xF, false))
#define KMX_RQ_SCAN_STEP32(ctrl, rows) v = op(KMX_RQ_DPP32(ident, v, ctrl, rows), v)
template <class Op>
__device__ __forceinline__ u32 wave_scan32(u32 v, const u32 ident, Op op) {
    KMX_RQ_SCAN_STEP32(0x111 /* row_shr:1 */, 0xF);
    KMX_RQ_SCAN_STEP32(0x112 /* row_shr:2 */, 0xF);
    KMX_RQ_SCAN_STEP32(0x114 /* row_shr:4 */, 0xF);
    KMX_RQ_SCAN_STEP32(0x118 /* row_shr:8 */, 0xF);
    KMX_RQ_SCAN_STEP32(0x142 /* row_bcast:15 */, 0xA);
    KMX_RQ_SCAN_STEP32(0x143 /* row_bcast:31 */, 0xC);
    return v;
}
#define KMX_RQ_SCAN_STEP64(ctrl, rows)                                                                   \
    v = op(((u64)KMX_RQ_DPP32((u32)(ident >> 32), (u32)(v >> 32), ctrl, rows) << 32) | KMX_RQ_DPP32((u32)ident, (u32)v, ctrl, rows), v)
template <class Op>
__device__ __forceinline__ u64 wave_scan64(u64 v, const u64 ident, Op op) {
    KMX_RQ_SCAN_STEP64(0x111, 0xF);
    KMX_RQ_SCAN_STEP64(0x112, 0xF);
    KMX_RQ_SCAN_STEP64(0x114, 0xF);
    KMX_RQ_SCAN_STEP64(0x118, 0xF);
    KMX_RQ_SCAN_STEP64(0x142, 0xA);
    KMX_RQ_SCAN_STEP64(0x143, 0xC);
    return v;
}

// the value of the lane before (lane 0: ident)
__device__ __forceinline__ u32 lane_before(u32 v, u32 ident, u32 lane) {
    const u32 o = __shfl_up(v, 1, WAVE);
    return lane ? o : ident;
}
__device__ __forceinline__ u64 lane_before(u64 v, u64 ident, u32 lane) {
    const u64 o = __shfl_up(v, 1, WAVE);
    return lane ? o : ident;
}

// max over the wave of a 64-bit value, wave-uniform (the shape of wave_sum, kmx_device.h)
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
    auto mx = [](u64 a, u64 b) { return a > b ? a : b; };
    v = mx(v, KMX_DPP64(v, 0xB1));
    v = mx(v, KMX_DPP64(v, 0x4E));
    v = mx(v, KMX_DPP64(v, 0x124));
    v = mx(v, KMX_DPP64(v, 0x128));
    return mx(mx(readlane64(v, 0), readlane64(v, 16)), mx(readlane64(v, 32), readlane64(v, 48)));
}

// the lowest lane whose flag is set (some lane's is)
__device__ __forceinline__ u32 first_lane(bool f) { return (u32)__builtin_ctzll(__ballot(f)); }

// The four bytes at positions p .. p + 4 of the read that starts at src (p may be negative by up to three, or lie past the read) as a
// dword, from the aligned dwords that hold them.  `phase` = the address of position p mod 4: the same for every lane and step of a
// read, whose positions differ by multiples of four.  A dword is loaded only if it holds a byte of the read, positions [0, L).
__device__ __forceinline__ u32 load4(uintptr_t src, u32 L, int64_t p, u32 phase) {
    const int64_t rp = p - (int64_t)phase;   // the position of the first aligned dword's byte 0
    u32 x0 = 0, x1 = 0;
    if (rp + 4 > 0 && rp < (int64_t)L) x0 = *reinterpret_cast<const u32*>(src + (uintptr_t)rp);
    if (phase != 0u && rp + 8 > 0 && rp + 4 < (int64_t)L) x1 = *reinterpret_cast<const u32*>(src + (uintptr_t)rp + 4u);
    return (u32)((((u64)x1 << 32) | x0) >> (8u * phase));
}

}  // namespace

__global__ void __launch_bounds__(WPR_THREADS) reads_quality_kernel(const ReadsQuality a) {
    __shared__ u64 wt[256];
    const bool weigh = a.weights != nullptr;
    if (weigh) wt[threadIdx.x] = a.weights[threadIdx.x];
    __syncthreads();
    const u32 lane = threadIdx.x & 63u;
    const u32 wv = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 stride = (u64)gridDim.x * WPR_WAVES;
    for (u64 r = (u64)blockIdx.x * WPR_WAVES + wv; r < a.n_reads; r += stride) {
        u64 off;
        const u32 L = read_span(a.offsets, a.read_len, r, off);
        const uintptr_t bsrc = reinterpret_cast<uintptr_t>(a.bases) + off, qsrc = reinterpret_cast<uintptr_t>(a.quals) + off;
        const uintptr_t dst = a.masked ? reinterpret_cast<uintptr_t>(a.masked) + off : bsrc;
        const u32 A = (u32)(dst & 3u);
        const u32 bphase = (u32)(bsrc - A) & 3u, qphase = (u32)(qsrc - A) & 3u;
        // what the steps carry (wave-uniform)
        int64_t Pc = 0, Mc = 0;            // the prefix sum at the step's first byte; the smallest prefix sum so far ...
        u32 Ac = 0;                        // ... and the last index that has it
        u64 V = 0;                         // the best D so far, at prefix index bstar, its minimum at astar
        u32 bstar = 0, astar = 0;
        u32 last_bad = 0;                  // 1 + the last position that is not GOOD (0: none)
        u32 run_len = 0, run_start = 0;
        // what a lane sums over the steps, reduced once behind them
        u64 l_q = 0, l_w = 0;              // its q; its weights
        u32 l_low = 0, l_win = 0, l_max = 0, l_minc = 0;   // ...; the largest q; 255 - the smallest
        const u32 span = L ? A + L : 0u;                      // (L < 2^31: the grid positions fit 32 bits)
        for (u32 s0 = 0; s0 < span; s0 += RQ_STEP) {
            const u32 g0 = s0 + lane * RQ_LANE;               // the lane's first byte on the grid; its position in the read is g0 - A
            const int64_t p0 = (int64_t)g0 - (int64_t)A;
            const u32 bw = load4(bsrc, L, p0, bphase), qw = load4(qsrc, L, p0, qphase);
            // ---- the first walk
            u32 vm = 0, gm = 0, ow = 0;
            int32_t sj[RQ_LANE];
            int32_t S = 0;
            u32 lb = 0;
#pragma unroll
            for (u32 j = 0; j < RQ_LANE; ++j) {
                const u32 g = g0 + j;
                const bool v = g >= A && g - A < L;
                const u32 p = g - A;
                const u32 b = (bw >> (8u * j)) & 0xFFu, qb = (qw >> (8u * j)) & 0xFFu;
                const u32 q = qb >= a.phred ? qb - a.phred : 0u;
                const bool lo = q < a.min_q;
                const bool good = v && !lo && is_acgt(b);
                ow |= (lo ? (u32)'N' : b) << (8u * j);
                sj[j] = v ? (int32_t)q - (int32_t)a.trim_q : 0;
                S += sj[j];
                if (v) {
                    vm |= 1u << j;
                    l_q += q;
                    l_low += lo ? 1u : 0u;
                    l_max = l_max > q ? l_max : q;
                    l_minc = l_minc > 255u - q ? l_minc : 255u - q;
                    if (!good) lb = p + 1u;
                    if (weigh) l_w += wt[qb];
                }
                if (good) gm |= 1u << j;
            }
            if (a.masked && vm) {
                uint8_t* const o = reinterpret_cast<uint8_t*>(dst - A + g0);
                if (vm == 0xFu) {
                    *reinterpret_cast<u32*>(o) = ow;
                } else {
#pragma unroll
                    for (u32 j = 0; j < RQ_LANE; ++j)
                        if (vm & (1u << j)) o[j] = (uint8_t)(ow >> (8u * j));
                }
            }
            // ---- the scans
            auto mx32 = [](u32 x, u32 y) { return x > y ? x : y; };
            const u32 lb_in = wave_scan32(lb, 0u, mx32);
            u32 lbr = mx32(lane_before(lb_in, 0u, lane), last_bad);
            const u32 S_in = wave_scan32((u32)S, 0u, [](u32 x, u32 y) { return x + y; });
            int32_t rel = (int32_t)(S_in - (u32)S);                 // the prefix sum at the lane's first byte, relative to the step
            u64 key = ~0ull;                                        // the lane's smallest prefix sum, the last of equal ones
            {
                int32_t t = rel;
#pragma unroll
                for (u32 j = 0; j < RQ_LANE; ++j) {
                    t += sj[j];
                    const u64 kj = ((u64)((u32)t + 0x80000000u) << 32) | (u32) ~(g0 + j - A + 1u);
                    if ((vm & (1u << j)) && kj < key) key = kj;
                }
            }
            const u64 key_in = wave_scan64(key, ~0ull, [](u64 x, u64 y) { return x < y ? x : y; });
            const u64 key_ex = lane_before(key_in, ~0ull, lane);
            int64_t M = Mc;
            u32 Ai = Ac;
            if (key_ex != ~0ull) {
                const int64_t m = Pc + (int64_t)(int32_t)((u32)(key_ex >> 32) - 0x80000000u);
                if (m <= M) {
                    M = m;
                    Ai = ~(u32)key_ex;
                }
            }
            // ---- the second walk
            int64_t P = Pc + rel;
            u64 bestD = 0;
            u32 bestb = 0, besta = 0, bestrun = 0, beststart = 0;
#pragma unroll
            for (u32 j = 0; j < RQ_LANE; ++j) {
                if (vm & (1u << j)) {
                    const u32 p = g0 + j - A;
                    P += sj[j];
                    if (P <= M) {
                        M = P;
                        Ai = p + 1u;
                    }
                    const u64 D = (u64)(P - M);
                    if (D > bestD) {
                        bestD = D;
                        bestb = p + 1u;
                        besta = Ai;
                    }
                    if (!(gm & (1u << j))) lbr = p + 1u;
                    const u32 run = p + 1u - lbr;
                    if (run > bestrun) {
                        bestrun = run;
                        beststart = lbr;
                    }
                    l_win += (a.k != 0u && run >= a.k) ? 1u : 0u;
                }
            }
            // ---- the wave's best, its sums, what the next step starts from
            const u64 Dmax = wave_max_u64(bestD);
            if (Dmax > V) {
                const u32 sel = first_lane(bestD == Dmax);
                V = Dmax;
                bstar = (u32)__builtin_amdgcn_readlane((int)bestb, (int)sel);
                astar = (u32)__builtin_amdgcn_readlane((int)besta, (int)sel);
            }
            const u32 rmax = wave_max_u32(bestrun);
            if (rmax > run_len) {
                const u32 sel = first_lane(bestrun == rmax);
                run_len = rmax;
                run_start = (u32)__builtin_amdgcn_readlane((int)beststart, (int)sel);
            }
            Pc += (int64_t)(int32_t)__builtin_amdgcn_readlane((int)S_in, 63);
            Mc = (int64_t)readlane64((u64)M, 63);
            Ac = (u32)__builtin_amdgcn_readlane((int)Ai, 63);
            last_bad = (u32)__builtin_amdgcn_readlane((int)lbr, 63);
            // (these ride in vector registers between the steps: with them the kernel's uniform state is past what
            // the scalar file holds, and the compiler spills scalars)
            asm volatile("" : "+v"(Pc), "+v"(Mc), "+v"(V), "+v"(astar), "+v"(bstar), "+v"(run_start));
        }
        if (!a.rows) continue;
        const u64 qsum = wave_sum(l_q), lw = wave_sum((u64)l_low | ((u64)l_win << 32)), weight = weigh ? wave_sum(l_w) : 0u;   // (low, windows < 2^31)
        const u64 low = lw & 0xFFFFFFFFull, wins = lw >> 32;
        const u32 q_max = wave_max_u32(l_max), q_minc = wave_max_u32(l_minc);
        if (lane < KMX_RQ_WORDS) {
            // the lane's word by the three bits of its number (three lane masks for the compiler to keep, not seven)
            static_assert(KMX_RQ_BASES == 0u && KMX_RQ_LOW == 1u && KMX_RQ_QSUM == 2u && KMX_RQ_WEIGHT == 3u && KMX_RQ_MINMAX == 4u &&
                          KMX_RQ_TRIM == 5u && KMX_RQ_RUN == 6u && KMX_RQ_WINDOWS == 7u && KMX_RQ_WORDS == 8u, "the order of a row's words");
            const u64 w_minmax = L ? (u64)(255u - q_minc) | ((u64)q_max << 32) : 0u;
            const u64 w_trim = V ? (u64)astar | ((u64)(bstar - astar) << 32) : 0u;
            const u64 w_run = run_len ? (u64)run_start | ((u64)run_len << 32) : 0u;
            const bool b0 = (lane & 1u) != 0u, b1 = (lane & 2u) != 0u, b2 = (lane & 4u) != 0u;
            const u64 w01 = b0 ? low : (u64)L, w23 = b0 ? weight : qsum, w45 = b0 ? w_trim : w_minmax, w67 = b0 ? wins : w_run;
            const u64 w = b2 ? (b1 ? w67 : w45) : (b1 ? w23 : w01);
            a.rows[r * KMX_RQ_WORDS + lane] = w;
        }
    }
}

hipError_t launch_reads_quality(const ReadsQuality& a, int n_cu, hipStream_t st) {
    hipLaunchKernelGGL(reads_quality_kernel, dim3(wave_per_read_grid(a.n_reads, n_cu)), dim3(WPR_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace kmx
