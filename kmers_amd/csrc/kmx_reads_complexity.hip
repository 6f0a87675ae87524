// kmx_reads_complexity.hip -- one pass over the bases of a batch of reads, no quality bytes and no table: kmx_reads_complexity.
// Poly-X tails and heads (the keep span), base composition, the neighbour pairs that differ, the DUST numerators of 64-base
// windows and the copy with the DUSTY windows turned to 'N'.  kmx.h has the contract (the poly-X rule, the windows, the eight
// words of a row); DESIGN 4.6.20 has the reasoning and the figures.
//
// A WAVE PER READ, A LANE PER BASE.  Every load and every store is of ONE BYTE, the lane's: no aligned dword is touched that
// holds no byte of the read, no byte outside the read is written, and no alignment of d_bases or d_masked is a case of its own.
// A wave's 64 byte accesses are consecutive, so they coalesce into one or two cache lines.  The read is walked three times, each
// walk exact for any length with its state carried in wave-uniform registers; the second and third see the lines the first brought.
// The window walk loads a window ahead of the one it works on.
//
// THE POLY WALKS come first (in place, the masked copy overwrites what they read).  The tail: 64 bases a step from the read's END,
// lane l holding position L - 64 (k + 1) + l.  One ballot per selected letter X turns the step into a plane word, bit l = "the
// base is X".  A lane owns the suffix that starts at its position: its mismatches are the zero bits of the word at and above its
// lane plus `carry`, the mismatches of everything behind the step.  The best suffix of a step is ONE wave max over the packed
// key (score + 2^40) << 6 | (63 - lane): inside a step the longer suffix is the lower lane.  The walk of a letter ends, exactly,
// once carry * err_den > err_num * L: every suffix still to come holds at least `carry` mismatches in at most L bases.  At a tenth a random 150-base read is done after one step.  The head is the
// mirror image from the front: prefixes, the zero bits at and below the lane, the longer prefix the higher lane.
//
// THE WINDOW WALK.  Window j is a wave: lane l holds base 32 j + l.  Three ballots -- the low bit of the code (byte >> 1) & 3, the
// high bit, "is one of ACGTacgt" -- give three plane words, and everything else about the window comes out of them:
//   composition and neighbours: scalar popcounts of the planes under the mask of the bases (pairs) no earlier window held;
//   the triplets: the six bit planes of the triplet code are lo, hi and their shifts by one and two, "counted" is
//   val & val >> 1 & val >> 2.  A lane compares its own six bits with the planes: the lanes that spell its triplet are a 64-bit
//   mask, c its popcount, and the sum of c - 1 over the counted lanes is 2 S.  One wave sum a window.
// The first 32 bases of a window lie in no later one, so they are stored behind it ('N' iff this window or the one before is
// DUSTY); the last window stores all its bases.  Every byte is stored once, by the wave that owns the read.
// No table, no LDS, no atomics, no scratch, no work buffer; a row is written by the eight low lanes.
// The bounds of a read, "is one of ACGTacgt" and the wave-per-read launch shape are the family's (kmx_reads_common.h).
#include "kmx_reads_common.h"

namespace kmx {

namespace {

constexpr u64 RX_BIAS = 1ull << 40;   // score + RX_BIAS > 0: |score| <= 2^31 + 256 * 2^31

// sum over the 64 lanes, returned wave-uniform (the shape of wave_max_u32, kmx_device.h)
__device__ __forceinline__ u32 wave_sum_u32(u32 v) {
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1 /* quad_perm:[1,0,3,2] */, 0xF, 0xF, true);
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E /* quad_perm:[2,3,0,1] */, 0xF, 0xF, true);
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x124 /* row_ror:4 */, 0xF, 0xF, true);
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x128 /* row_ror:8 */, 0xF, 0xF, true);
    return (u32)__builtin_amdgcn_readlane((int)v, 0) + (u32)__builtin_amdgcn_readlane((int)v, 16) +
           (u32)__builtin_amdgcn_readlane((int)v, 32) + (u32)__builtin_amdgcn_readlane((int)v, 48);
}

// max over the wave of a 64-bit value, wave-uniform (wave_max_u64 of kmx_reads_quality.hip)
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
    auto mx = [](u64 a, u64 b) { return a > b ? a : b; };
    v = mx(v, KMX_DPP64(v, 0xB1));
    v = mx(v, KMX_DPP64(v, 0x4E));
    v = mx(v, KMX_DPP64(v, 0x124));
    v = mx(v, KMX_DPP64(v, 0x128));
    return mx(mx(readlane64(v, 0), readlane64(v, 16)), mx(readlane64(v, 32), readlane64(v, 48)));
}

__device__ __forceinline__ u64 low_bits(u32 n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }

// The best poly-X end of the read at src[0 .. L), L >= 1, over the letters of `letters`: the word of KMX_RX_TAIL / KMX_RX_HEAD.
// TAIL: suffixes, walked from the end; otherwise prefixes, walked from the front.
template <bool TAIL>
__device__ __forceinline__ u64 poly_end(const uint8_t* src, u32 L, u32 letters, const ReadsComplexity& a, u32 lane) {
    u32 carry[4] = {0, 0, 0, 0};       // per letter: the bases that are not X in the steps behind
    // The best end so far over all letters: score + RX_BIAS (0: none), its length | (bit index + 1) << 32.  One best serves: the
    // order is (score, length) whatever the letter, a step takes the letters in ascending order and a later one must be better.
    u64 best_s = 0, best = 0;
    u32 alive = letters;
    const u64 room = (u64)a.err_num * L;   // the mismatches * err_den that any end of this read may hold
    for (u32 k0 = 0; k0 < L && alive; k0 += 64u) {
        // the lane's position: the step covers [L - k0 - 64, L - k0) or [k0, k0 + 64)
        const int64_t p = TAIL ? (int64_t)L - (int64_t)k0 - 64 + (int64_t)lane : (int64_t)k0 + (int64_t)lane;
        const bool in = p >= 0 && p < (int64_t)L;
        const u32 u = in ? (u32)src[p] & 0xDFu : 0u;
        const u32 n = TAIL ? k0 + 64u - lane : k0 + lane + 1u;   // the length of the lane's suffix / prefix (in: n <= L)
#pragma unroll
        for (u32 x = 0; x < 4u; ++x) {
            if (!(alive & (1u << x))) continue;
            const bool is_x = u == (u32)"ACGT"[x];
            const u64 word = __ballot(is_x);
            const u64 inside = __ballot(in);
            const u64 miss = ~word & inside;
            const u32 m = carry[x] + (u32)__popcll(TAIL ? miss >> lane : miss & low_bits(lane + 1u));
            const bool ok = is_x && n >= a.min_len && (u64)m * a.err_den <= (u64)a.err_num * n;
            if (__ballot(ok)) {
                const u64 s = RX_BIAS + n - (u64)(a.penalty + 1u) * m;
                const u64 top = wave_max_u64(ok ? (s << 6) | (TAIL ? 63u - lane : lane) : 0u);
                const u32 l = TAIL ? 63u - (u32)(top & 63u) : (u32)(top & 63u);
                const u32 len = TAIL ? k0 + 64u - l : k0 + l + 1u;
                if ((top >> 6) > best_s || ((top >> 6) == best_s && len > (u32)best)) {
                    best_s = top >> 6;
                    best = (u64)len | ((u64)(x + 1u) << 32);
                }
            }
            carry[x] += (u32)__popcll(miss);
            if ((u64)carry[x] * a.err_den > room) alive &= ~(1u << x);   // no longer end can qualify
        }
    }
    return best;
}

}  // namespace

__global__ void __launch_bounds__(WPR_THREADS) reads_complexity_kernel(const ReadsComplexity a) {
    const u32 lane = threadIdx.x & 63u;
    const u32 wv = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 stride = (u64)gridDim.x * WPR_WAVES;
    for (u64 r = (u64)blockIdx.x * WPR_WAVES + wv; r < a.n_reads; r += stride) {
        u64 off;
        const u32 L = read_span(a.offsets, a.read_len, r, off);
        const uint8_t* const src = a.bases + off;
        uint8_t* const dst = a.masked ? a.masked + off : nullptr;
        // (the bases of the first window are asked for before the poly walks, and those of every other window a window ahead: a window
        // is a chain of dependent steps behind its load, and with the load where its bytes are wanted a read waited once per window)
        const u32 W = L == 0u ? 0u : L <= 64u ? 1u : (L - 64u + 31u) / 32u + 1u;
        u32 b_ahead = lane < L ? (u32)src[lane] : 0u;
        // ---- the poly-X ends (before a byte of the read is written: in place they are the same bytes)
        u64 w_tail = 0, w_head = 0;
        if (a.rows && L) {
            if (a.tail_bases) w_tail = poly_end<true>(src, L, a.tail_bases, a, lane);
            if (a.head_bases) w_head = poly_end<false>(src, L, a.head_bases, a, lane);
        }
        // ---- the windows
        u32 n_a = 0, n_c = 0, n_g = 0, n_t = 0, n_pairs = 0, n_diff = 0, s_max = 0, n_dusty = 0;
        bool dusty_before = false;
        for (u32 j = 0; j < W; ++j) {
            const u32 i = 32u * j + lane;   // (32 W + 63 < L + 127: no wrap)
            const bool in = i < L;
            const u32 b = b_ahead;
            if (j + 1u < W) b_ahead = i + 32u < L ? (u32)src[i + 32u] : 0u;   // (no byte of the next window is stored by this one)
            const u32 c = (b >> 1) & 3u;    // A 0, C 1, T 2, G 3, either case
            const bool valid = in && is_acgt(b);
            const u64 val = __ballot(valid), lo = __ballot(valid && (c & 1u)), hi = __ballot(valid && (c & 2u));
            // the bases and the pairs (at their first lane) that no window before this one held
            const u64 fresh = j ? ~0ull << 32 : ~0ull, fresh_pairs = j ? ~0ull << 31 : ~0ull;
            n_a += (u32)__popcll(val & ~lo & ~hi & fresh);
            n_c += (u32)__popcll(lo & ~hi & fresh);
            n_t += (u32)__popcll(hi & ~lo & fresh);
            n_g += (u32)__popcll(hi & lo & fresh);
            const u64 pairs = val & (val >> 1) & fresh_pairs;
            n_pairs += (u32)__popcll(pairs);
            n_diff += (u32)__popcll(pairs & ((lo ^ (lo >> 1)) | (hi ^ (hi >> 1))));
            // the lanes that spell the lane's triplet
            u64 same = val & (val >> 1) & (val >> 2);   // counted: bits past the window's last base are 0
            const bool counted = (same >> lane) & 1u;
            const u32 tl = (u32)(lo >> lane), th = (u32)(hi >> lane);
#pragma unroll
            for (u32 d = 0; d < 3u; ++d) {
                same &= ~((lo >> d) ^ (0ull - (u64)((tl >> d) & 1u)));
                same &= ~((hi >> d) ^ (0ull - (u64)((th >> d) & 1u)));
            }
            const u32 S = wave_sum_u32(counted ? (u32)__popcll(same) - 1u : 0u) >> 1;
            const bool dusty = S > a.dust_max;
            s_max = S > s_max ? S : s_max;
            n_dusty += dusty ? 1u : 0u;
            if (dst && in) {
                if (lane < 32u) {
                    dst[i] = (uint8_t)(dusty || dusty_before ? (u32)'N' : b);
                } else if (j + 1u == W) {
                    dst[i] = (uint8_t)(dusty ? (u32)'N' : b);
                }
            }
            dusty_before = dusty;
        }
        if (a.rows && lane < KMX_RX_WORDS) {
            static_assert(KMX_RX_KEEP == 0u && KMX_RX_BASES == 1u && KMX_RX_TAIL == 2u && KMX_RX_HEAD == 3u && KMX_RX_AC == 4u &&
                          KMX_RX_GT == 5u && KMX_RX_DIFF == 6u && KMX_RX_DUST == 7u && KMX_RX_WORDS == 8u, "the order of a row's words");
            const u32 t = (u32)w_tail, h = (u32)w_head;
            const u64 w_keep = (u64)h + t >= L ? 0u : (u64)h | ((u64)(L - h - t) << 32);
            // (the lane masks of the word's choice are made here, per read: hoisted out of the loop over the reads they are six
            // scalar registers held across all three walks, which the scalar file does not have to spare)
            u32 ln = lane;
            asm volatile("" : "+v"(ln));
            const bool b0 = (ln & 1u) != 0u, b1 = (ln & 2u) != 0u, b2 = (ln & 4u) != 0u;
            const u64 w01 = b0 ? (u64)L : w_keep, w23 = b0 ? w_head : w_tail;
            const u64 w45 = b0 ? (u64)n_g | ((u64)n_t << 32) : (u64)n_a | ((u64)n_c << 32);
            const u64 w67 = b0 ? (u64)s_max | ((u64)n_dusty << 32) : (u64)n_diff | ((u64)n_pairs << 32);
            a.rows[r * KMX_RX_WORDS + lane] = b2 ? (b1 ? w67 : w45) : (b1 ? w23 : w01);
        }
    }
}

hipError_t launch_reads_complexity(const ReadsComplexity& a, int n_cu, hipStream_t st) {
    hipLaunchKernelGGL(reads_complexity_kernel, dim3(wave_per_read_grid(a.n_reads, n_cu)), dim3(WPR_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace kmx
