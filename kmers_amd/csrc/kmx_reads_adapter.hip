// kmx_reads_adapter.hip -- adapter read-through found on the device: kmx_reads_adapter (known 3' adapters, with mismatches and
// wildcards) and kmx_reads_pair_overlap (the overlap of two mates: the insert size without knowing the adapter).  kmx.h has the
// contracts (a hit, the tie rules, the four words of a row); DESIGN 4.6.16 has the reasoning and the figures.
//
// Both are a Hamming distance between two base strings at every relative shift, on BIT PLANES.  A WAVE PER READ (PAIR).  The wave
// turns 64 consecutive bases into three 64-bit words with three ballots -- the low bit of the base's code, the high bit, "is one of
// ACGTacgt" -- lane l holding base l: the words are wave-uniform.  The code is (byte >> 1) & 3 (A 0, C 1, T 2, G 3; the case bit
// falls out), so the complement is the high bit flipped.  A lane owns one candidate shift: it takes the 64 bases at its shift out
// of two neighbouring plane words with a funnel shift, and the mismatches of 64 bases are
//     popcount(((lo ^ lo') | (hi ^ hi') | ~valid) & mask).
// THE DWORD GRID.  A read is laid on the grid of aligned dwords that holds it: position q of the grid is the byte at g + q, g the
// aligned address at or below the read's first byte, so the read is q in [A, A + L) with A < 4 (for a reverse complement the grid
// runs down from the aligned address at or above the read's end).  Plane words, shifts and candidate positions all count in q.  A
// lane loads ONE aligned dword per 256 positions -- a step, one coalesced 256-byte load per wave, and only dwords that hold a byte
// of the read -- and the byte of position 64 c + lane comes out of lane 16 c + lane / 4 by a lane permute: the hot shape (100 to
// 250 bases) costs one load's latency per read, not one per plane word.
//
// kmx_reads_adapter: the adapters ride in the kernel arguments as plane words (at most 8 of at most 64 bases: one word per plane),
// with `care` = the positions that are inside the adapter and not a wildcard.  The wave walks the read 64 positions at a time and
// keeps two plane words, the current and the next: an adapter is at most one word long, so the window at q = q0 + lane lies in
// them.  Exact for any length (the dwords of the step after the current one are requested a step ahead); the leftmost hit of a
// step is a ballot and a count of trailing zeros.
// kmx_reads_pair_overlap: the planes of mate 1 and of the reverse complement of mate 2 -- read back to front and complemented as
// it is loaded, no bit reversal -- go to LDS once (at most 1024 bases: 17 words and a zero word behind them, per plane), a lane
// owns a shift d and walks the overlap word by word; it stops once it is past max_mism, which only a non-hit can be.
// No atomics, no scratch, no work buffer; a row is written by the four low lanes of the one wave that owns the read.
// The bounds of a read, "is one of ACGTacgt" and the wave-per-read launch shape are the family's (kmx_reads_common.h).
#include "kmx_reads_common.h"

namespace kmx {

namespace {

constexpr u32 RP_WORDS_MAX = KMX_RP_MAX_LEN / 64u + 2u;   // the plane words of a mate on its grid (A + L <= 1027) and the zero word behind them

struct Planes {
    u64 lo, hi, val;
};

// A read on its dword grid (see above).  span = A + L, 0 for an empty read.
struct Grid {
    uintptr_t g;
    u32 A, span;
};
template <bool RC>
__device__ __forceinline__ Grid grid_of(uintptr_t src, u32 L) {
    const uintptr_t end = src + L;
    const uintptr_t g = RC ? (end + 3u) & ~(uintptr_t)3 : src & ~(uintptr_t)3;
    const u32 A = (u32)(RC ? g - end : src - g);
    return Grid{g, A, L ? A + L : 0u};
}

// The lane's dword of step s: grid positions 256 s + 4 lane .. + 3 in its bytes 0 .. 3 (RC: the dword below g, its bytes swapped).
// Loaded only if it holds a byte of the read; 0 otherwise.
template <bool RC>
__device__ __forceinline__ u32 load_step(const Grid& G, u32 s, u32 lane) {
    const u32 q = 256u * s + 4u * lane;
    u32 w = 0;
    if (q + 4u > G.A && q < G.span) {
        w = *reinterpret_cast<const u32*>(RC ? G.g - 4u - q : G.g + q);
        if (RC) w = __builtin_bswap32(w);
    }
    return w;
}

// Grid positions [q0, q0 + 64) (q0 a multiple of 64 inside the step whose dwords the wave holds in dw) as plane words, lane l
// bringing position q0 + l; positions outside the read are not valid.  RC: the bases complemented.
template <bool RC>
__device__ __forceinline__ Planes planes64(u32 dw, const Grid& G, u32 q0, u32 lane) {
    const u32 v = (u32)__shfl((int)dw, (int)(16u * ((q0 >> 6) & 3u) + (lane >> 2)), WAVE);
    const u32 b = (v >> (8u * (lane & 3u))) & 0xFFu;
    const u32 q = q0 + lane;
    const bool ok = q >= G.A && q < G.span && is_acgt(b);
    const u32 c = ((b >> 1) & 3u) ^ (RC ? 2u : 0u);
    return Planes{__ballot(ok && (c & 1u)), __ballot(ok && (c & 2u)), __ballot(ok)};
}

// bits [sh, sh + 64) of the 128 bits hi:lo (sh < 64)
__device__ __forceinline__ u64 funnel(u64 lo, u64 hi, u32 sh) { return sh ? (lo >> sh) | (hi << (64u - sh)) : lo; }
__device__ __forceinline__ u64 low_bits(u32 n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }

}  // namespace

__global__ void __launch_bounds__(WPR_THREADS) reads_adapter_kernel(const ReadsAdapter a) {
    const u32 lane = threadIdx.x & 63u;
    const u32 wv = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 stride = (u64)gridDim.x * WPR_WAVES;
    const u32 all = (1u << a.n_adapters) - 1u;
    for (u64 r = (u64)blockIdx.x * WPR_WAVES + wv; r < a.n_reads; r += stride) {
        u64 off;
        const u32 L = read_span(a.offsets, a.read_len, r, off);
        const uintptr_t src = reinterpret_cast<uintptr_t>(a.bases) + off;
        bool found = false;
        u32 keep = L, hits = 0;
        u64 hit_word = 0;
        const Grid G = grid_of<false>(src, L);
        if (G.span) {
            u32 dw = load_step<false>(G, 0u, lane), dw_next = load_step<false>(G, 1u, lane);   // (a step ahead: a long read waits once)
            Planes cur = planes64<false>(dw, G, 0u, lane);
            for (u32 q0 = 0; q0 < G.span; q0 += 64u) {
                const u32 qn = q0 + 64u;
                Planes nxt{0, 0, 0};
                if (qn < G.span) {
                    if ((qn & 255u) == 0u) {
                        dw = dw_next;
                        dw_next = load_step<false>(G, (qn >> 8) + 1u, lane);
                    }
                    nxt = planes64<false>(dw, G, qn, lane);
                }
                const u32 q = q0 + lane;
                const u32 rem = q >= G.A && q < G.span ? G.span - q : 0u;   // the bases from the lane's position to the read's end
                const u64 wlo = funnel(cur.lo, nxt.lo, lane), whi = funnel(cur.hi, nxt.hi, lane), wbad = ~funnel(cur.val, nxt.val, lane);
                u32 first = 64u, first_a = 0, first_m = 0;
                for (u32 i = 0; i < a.n_adapters; ++i) {
                    const u32 n = a.len[i] < rem ? a.len[i] : rem;   // (rem == 0: n == 0 < min_overlap)
                    const u32 m = (u32)__popcll(((wlo ^ a.lo[i]) | (whi ^ a.hi[i]) | wbad) & a.care[i] & low_bits(n));
                    const bool hit = n >= a.min_overlap && (u64)m * a.err_den <= (u64)a.err_num * n;
                    const u64 bal = __ballot(hit);
                    if (bal) {
                        hits |= 1u << i;
                        const u32 f = (u32)__builtin_ctzll(bal);
                        if (!found && f < first) {   // (of the adapters that hit at one p the first stays)
                            first = f;
                            first_a = i;
                            first_m = (u32)__builtin_amdgcn_readlane((int)m, (int)f);
                        }
                    }
                }
                if (!found && first < 64u) {
                    found = true;
                    keep = q0 + first - G.A;
                    const u32 n = a.len[first_a] < L - keep ? a.len[first_a] : L - keep;
                    hit_word = (u64)(first_a + 1u) | ((u64)n << 16) | ((u64)first_m << 32);
                }
                if (hits == all) break;   // (then `found` holds, and no word of the row can change any more)
                cur = nxt;
            }
        }
        if (lane < KMX_RA_WORDS) {
            static_assert(KMX_RA_KEEP == 0u && KMX_RA_HIT == 1u && KMX_RA_BASES == 2u && KMX_RA_HITS == 3u && KMX_RA_WORDS == 4u,
                          "the order of a row's words");
            const bool b0 = (lane & 1u) != 0u, b1 = (lane & 2u) != 0u;
            const u64 w01 = b0 ? hit_word : (u64)keep << 32, w23 = b0 ? (u64)hits : (u64)L;
            a.rows[r * KMX_RA_WORDS + lane] = b1 ? w23 : w01;
        }
    }
}

__global__ void __launch_bounds__(WPR_THREADS) reads_pair_overlap_kernel(const ReadsPairOverlap a) {
    __shared__ u64 planes[WPR_WAVES][2][3][RP_WORDS_MAX];
    const u32 lane = threadIdx.x & 63u;
    const u32 wv = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 stride = (u64)gridDim.x * WPR_WAVES;
    u64(*const X)[RP_WORDS_MAX] = planes[wv][0];
    u64(*const Y)[RP_WORDS_MAX] = planes[wv][1];
    // what one lane wrote the others read: the wave's own barrier (the waves of a block share nothing)
    auto wave_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    for (u64 r = (u64)blockIdx.x * WPR_WAVES + wv; r < a.n_reads; r += stride) {
        u64 off1, off2;
        const u32 L1 = read_span(a.offsets1, a.read_len1, r, off1), L2 = read_span(a.offsets2, a.read_len2, r, off2);
        const uintptr_t src1 = reinterpret_cast<uintptr_t>(a.bases1) + off1, src2 = reinterpret_cast<uintptr_t>(a.bases2) + off2;
        u32 best_n = 0, best_i = 0, best_m = 0;
        if (L1 && L2 && L1 <= KMX_RP_MAX_LEN && L2 <= KMX_RP_MAX_LEN) {
            const Grid G1 = grid_of<false>(src1, L1), G2 = grid_of<true>(src2, L2);
            u32 dx = load_step<false>(G1, 0u, lane), dy = load_step<true>(G2, 0u, lane);   // (both mates' first steps in flight at once)
            wave_sync();   // (the reads of the pair before are done)
            // word c of every plane, c = 0 .. ceil(span / 64): the last one holds no base and is zero
            for (u32 q0 = 0; q0 < G1.span + 64u; q0 += 64u) {
                if (q0 && (q0 & 255u) == 0u) dx = load_step<false>(G1, q0 >> 8, lane);
                const Planes w = planes64<false>(dx, G1, q0, lane);
                if (lane == 0) {
                    X[0][q0 >> 6] = w.lo;
                    X[1][q0 >> 6] = w.hi;
                    X[2][q0 >> 6] = w.val;
                }
            }
            for (u32 q0 = 0; q0 < G2.span + 64u; q0 += 64u) {
                if (q0 && (q0 & 255u) == 0u) dy = load_step<true>(G2, q0 >> 8, lane);
                const Planes w = planes64<true>(dy, G2, q0, lane);
                if (lane == 0) {
                    Y[0][q0 >> 6] = w.lo;
                    Y[1][q0 >> 6] = w.hi;
                    Y[2][q0 >> 6] = w.val;
                }
            }
            wave_sync();
            const u32 total = L1 + L2 - 1u;   // the shifts d = t - (L2 - 1), t in [0, total): the insert size is t + 1
            for (u32 t0 = 0; t0 < total; t0 += 64u) {
                const u32 t = t0 + lane;
                const u32 xs = t >= L2 ? t - (L2 - 1u) : 0u, ys = t < L2 ? L2 - 1u - t : 0u;   // the first base compared, of X and of Y
                u32 n = 0, m = 0;
                bool hit = false;
                if (t < total) {
                    n = L1 - xs < L2 - ys ? L1 - xs : L2 - ys;
                    if (n >= a.min_overlap) {
                        for (u32 w = 0; w < n && m <= a.max_mism; w += 64u) {
                            const u32 xq = G1.A + xs + w, yq = G2.A + ys + w;   // on the mates' grids
                            const u32 xi = xq >> 6, xsh = xq & 63u, yi = yq >> 6, ysh = yq & 63u;
                            const u64 xlo = funnel(X[0][xi], X[0][xi + 1u], xsh), xhi = funnel(X[1][xi], X[1][xi + 1u], xsh);
                            const u64 xv = funnel(X[2][xi], X[2][xi + 1u], xsh);
                            const u64 ylo = funnel(Y[0][yi], Y[0][yi + 1u], ysh), yhi = funnel(Y[1][yi], Y[1][yi + 1u], ysh);
                            const u64 yv = funnel(Y[2][yi], Y[2][yi + 1u], ysh);
                            m += (u32)__popcll(((xlo ^ ylo) | (xhi ^ yhi) | ~(xv & yv)) & low_bits(n - w));
                        }
                        hit = m <= a.max_mism && (u64)m * a.err_den <= (u64)a.err_num * n;
                    }
                }
                // the largest n, of equal ones the largest d: the steps come in ascending d, so a later step wins a tie
                const u32 nmax = wave_max_u32(hit ? n : 0u);
                if (nmax && nmax >= best_n) {
                    const u32 imax = wave_max_u32(hit && n == nmax ? t + 1u : 0u);
                    best_n = nmax;
                    best_i = imax;
                    best_m = (u32)__builtin_amdgcn_readlane((int)m, (int)(imax - 1u - t0));
                }
            }
        }
        if (lane < KMX_RP_WORDS) {
            static_assert(KMX_RP_INSERT == 0u && KMX_RP_OVERLAP == 1u && KMX_RP_KEEP1 == 2u && KMX_RP_KEEP2 == 3u && KMX_RP_WORDS == 4u,
                          "the order of a row's words");
            const u32 k1 = best_n && best_i < L1 ? best_i : L1, k2 = best_n && best_i < L2 ? best_i : L2;
            const bool b0 = (lane & 1u) != 0u, b1 = (lane & 2u) != 0u;
            const u64 w01 = b0 ? (u64)best_n | ((u64)best_m << 32) : (u64)best_i, w23 = (u64)(b0 ? k2 : k1) << 32;
            a.rows[r * KMX_RP_WORDS + lane] = b1 ? w23 : w01;
        }
    }
}

hipError_t launch_reads_adapter(const ReadsAdapter& a, int n_cu, hipStream_t st) {
    hipLaunchKernelGGL(reads_adapter_kernel, dim3(wave_per_read_grid(a.n_reads, n_cu)), dim3(WPR_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_reads_pair_overlap(const ReadsPairOverlap& a, int n_cu, hipStream_t st) {
    hipLaunchKernelGGL(reads_pair_overlap_kernel, dim3(wave_per_read_grid(a.n_reads, n_cu)), dim3(WPR_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace kmx
