// kmx_reads_merge.hip -- overlapping mate pairs merged into consensus reads: kmx_reads_pair_merge.  kmx.h has the contract (which
// pairs merge, the four classes of an overlap position, the words of a row); DESIGN 4.6.17 has the reasoning and the figures.
//
// Plan (its prologue is the family's, kmx_reads_plan.h; the length between two offsets and the wave-per-read launch shape are
// kmx_reads_common.h's).  One length per pair -- the insert word where the pair merges, 0 otherwise -- out of two offset pairs and the insert
// word.  A thread plans eight consecutive pairs, a block 2048: the count kernel sums merged pairs and bases per block, one block
// scans the two arrays of partial sums (the count family's scan_single_kernel) and the two totals come back to the host with the
// first and last offset of both batches: one round trip, all a count-only call without rows costs.  The write kernel computes the
// lengths again, scans them over the block and writes one output offset per PAIR: the output batch has as many reads as there are
// pairs.
//
// Merge.  A WAVE PER PAIR, built around the output: the merged read is laid on the grid of aligned dwords of d_out_bases that holds
// it, a lane owns one dword -- four consecutive positions i of the merged read -- per step of 256 positions, and stores it with
// one dword store (the two edges byte by byte: no byte outside the read is written).  The four bytes of mate 1 at i, and the four
// of mate 2 that the reverse complement brings there (the bytes at L2 - 4 - (i - d), swapped), come out of the two aligned dwords
// that hold them with one byte alignment; the two dword positions are clamped to the dwords that hold a byte the merged read uses,
// so no other dword is loaded and the loads take no branch.  The quality bytes likewise.  "Is one of ACGTacgt", the complement,
// "the same letter", the coverage and the choice of base and quality byte are SWAR on bytes of ones (no booleans: in a wave of 64
// each one alive is a pair of scalar registers); the quality arithmetic is per byte.  The quality bytes go out as a dword where
// d_out_quals has the alignment of d_out_bases mod 4 (two allocations always have), byte by byte otherwise.  The five class counts
// of a row are popcounts of the masks, packed into two registers per lane and summed over the wave once per pair.  The six words of
// a pair are one load of six lanes, requested a pair ahead.  No LDS, no atomics, no scratch; a row is written by the four low lanes
// of the wave that owns the pair.
#include "kmx_reads_plan.h"

namespace kmx {

namespace {

// The WORDS of pair r, six u64: where mate 1 begins and ends in d_bases, where mate 2 does, the insert word, the pair's output offset
// (the write and the merge only).  For uniform reads the first four are r and r + 1 times the read length.
constexpr u32 W_B1 = 0, W_E1 = 1, W_B2 = 2, W_E2 = 3, W_INSERT = 4, W_OUT = 5, W_WORDS = 6;
__device__ __forceinline__ u64 pair_word(const ReadsPairMerge& a, u64 r, u32 w, bool out) {
    if (w < W_INSERT) {
        const u64* const o = w < W_B2 ? a.offsets1 : a.offsets2;
        const u64 i = r + (w & 1u);
        return o ? o[i] : i * (u64)(w < W_B2 ? a.read_len1 : a.read_len2);
    }
    if (w == W_INSERT) return a.insert[r * a.insert_stride];
    return out && w == W_OUT ? a.out_offsets[r] : 0u;
}

// the mates of a pair (their lengths: span_len) and the length of its merged read: the insert word if the pair merges (kmx.h), else 0
struct Pair {
    u64 off1, off2;
    u32 L1, L2, I;
};
__device__ __forceinline__ Pair pair_from(u64 b1, u64 e1, u64 b2, u64 e2, u64 insert) {
    Pair p{b1, b2, span_len(b1, e1), span_len(b2, e2), 0u};
    const bool ok = p.L1 >= 1u && p.L2 >= 1u && p.L1 <= KMX_RP_MAX_LEN && p.L2 <= KMX_RP_MAX_LEN && insert > 0u && insert < (u64)p.L1 + p.L2;
    p.I = ok ? (u32)insert : 0u;
    return p;
}
__device__ __forceinline__ Pair pair_of(const ReadsPairMerge& a, u64 r) {
    return pair_from(pair_word(a, r, W_B1, false), pair_word(a, r, W_E1, false), pair_word(a, r, W_B2, false), pair_word(a, r, W_E2, false),
                     pair_word(a, r, W_INSERT, false));
}

// partial[b] = merged pairs of block b, partial[n_blocks + b] = their bases; tail[2 .. 6) = first and last offset of batch 1, of batch 2
__global__ void __launch_bounds__(CT) reads_merge_plan_count_kernel(const ReadsPairMerge a, u64* __restrict__ partial, u64 n_blocks,
                                                                    u64* __restrict__ tail) {
    plan_count(
        a.n_reads, partial, n_blocks,
        [&a](u64 r) {
            const u32 len = pair_of(a, r).I;
            return PlanRow{len != 0u, len};
        },
        [&a, tail] {
            tail[2] = a.offsets1 ? a.offsets1[0] : 0u;
            tail[3] = a.offsets1 ? a.offsets1[a.n_reads] : 0u;
            tail[4] = a.offsets2 ? a.offsets2[0] : 0u;
            tail[5] = a.offsets2 ? a.offsets2[a.n_reads] : 0u;
        });
}

// out_offsets[r] for every pair r; out_offsets[n_reads] = n_bases (tail[1]: the scanned total)
__global__ void __launch_bounds__(CT) reads_merge_plan_write_kernel(const ReadsPairMerge a, const u64* __restrict__ partial, u64 n_blocks,
                                                                    const u64* __restrict__ tail) {
    __shared__ u64 sh[CT];
    const u64 i0 = (u64)blockIdx.x * ROWS + (u64)threadIdx.x * RPT;
    u32 len[RPT];
    u64 bytes = 0;
#pragma unroll
    for (u32 j = 0; j < RPT; ++j) {
        len[j] = i0 + j < a.n_reads ? pair_of(a, i0 + j).I : 0u;
        bytes += len[j];
    }
    u64 tot;
    u64 b = partial[n_blocks + blockIdx.x] + block_exscan(bytes, sh, &tot);
#pragma unroll
    for (u32 j = 0; j < RPT; ++j) {
        if (i0 + j < a.n_reads) a.out_offsets[i0 + j] = b;
        b += len[j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.out_offsets[a.n_reads] = tail[1];
}

// a byte of ones for every byte k of a dword whose position i0 + k lies in [lo, hi)
__device__ __forceinline__ u32 cover(int i0, int lo, int hi) {
    auto low = [i0](int at) {   // the bytes k with i0 + k < at
        const int n = at - i0;
        return n >= 4 ? ~0u : ~(~0u << (8 * (n < 0 ? 0 : n)));
    };
    return low(hi) & ~low(lo);
}

// the bytes of w whose position i0 + k lies in [0, len) go to dst[i0 + k]: one dword store where all four do and `dword` says the
// address is aligned, byte by byte otherwise
__device__ __forceinline__ void store4(uint8_t* dst, int i0, u32 len, u32 w, bool dword) {
    if (dword && i0 >= 0 && (u32)i0 + 4u <= len) {
        *reinterpret_cast<u32*>(dst + i0) = w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k >= 0 && (u32)(i0 + k) < len) dst[i0 + k] = (uint8_t)(w >> (8 * k));
    }
}

}  // namespace

// QUALS: the mates have quality bytes (without: every quality byte reads as 0, so every q is 0).  OUT: the batch is written (without: the rows alone).
template <bool QUALS, bool OUT>
__global__ void __launch_bounds__(WPR_THREADS) reads_merge_kernel(const ReadsPairMerge a) {
    const u32 lane = threadIdx.x & 63u;
    const u32 wv = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 stride = (u64)gridDim.x * WPR_WAVES;
    // Lane w < 6 loads word w of a pair, so the six words of a pair are ONE load of the wave, and those of the NEXT pair are requested
    // before this pair's bytes: a wave then waits for memory once per pair, not three times in a row (words, output offset, bytes).
    auto lane_word = [&](u64 pair) { return lane < W_WORDS && pair < a.n_reads ? pair_word(a, pair, lane, OUT) : 0u; };
    u64 r = (u64)blockIdx.x * WPR_WAVES + wv;
    u64 next = lane_word(r);
    for (; r < a.n_reads; r += stride) {
        const u64 cur = next;
        next = lane_word(r + stride);
        const Pair p = pair_from(readlane64(cur, W_B1), readlane64(cur, W_E1), readlane64(cur, W_B2), readlane64(cur, W_E2),
                                 readlane64(cur, W_INSERT));
        const u64 oo = readlane64(cur, W_OUT);
        const u32 I = p.I;
        u32 n_ov = 0;
        u64 cnt = 0;   // 12-bit fields: DIS, DIS taken from mate 2, DIS with qx == qy, ONE, NONE (each at most 1024)
        u32 cnt_a = 0, cnt_b = 0;   // the lane's share: DIS | taken << 12 | NONE << 24 and ties | ONE << 12 (a lane sees at most 36 positions)
        if (I) {
            const int d = (int)I - (int)p.L2;
            const u32 y0 = d > 0 ? (u32)d : 0u;        // Y covers [y0, I)
            const u32 x1 = p.L1 < I ? p.L1 : I;        // X covers [0, x1)
            const u32 l2 = p.L2 < I ? p.L2 : I;        // the bytes of mate 2 that are used: its first l2
            n_ov = x1 - y0;
            uint8_t* const ob = OUT ? a.out_bases + oo : nullptr;
            uint8_t* const oq = OUT && QUALS && a.out_quals ? a.out_quals + oo : nullptr;
            const u32 A = (u32)(reinterpret_cast<uintptr_t>(ob) & 3u);   // the merged read is positions [A, A + I) of the output's dword grid
            const bool oq_dword = ((reinterpret_cast<uintptr_t>(ob) ^ reinterpret_cast<uintptr_t>(oq)) & 3u) == 0u;
            for (u32 g0 = 0; g0 < A + I; g0 += 256u) {
                const int i0 = (int)(g0 + 4u * lane) - (int)A;   // the lane's positions i0 .. i0 + 3 of the merged read
                if (i0 + 3 < 0 || i0 >= (int)I) continue;
                const int yat = (int)p.L2 - 4 - (i0 - d);           // Y[i0 - d + k] is the complement of byte yat + 3 - k of mate 2
                const u32 x = load4(a.bases1 + p.off1, i0, x1);
                const u32 yr = __builtin_bswap32(load4(a.bases2 + p.off2, yat, l2));
                u32 qxw = 0, qyw = 0;
                if (QUALS) {
                    qxw = load4(a.quals1 + p.off1, i0, x1);
                    qyw = __builtin_bswap32(load4(a.quals2 + p.off2, yat, l2));
                }
                u32 x_at, x_cg, y_at, y_cg;
                letters(x, x_at, x_cg);
                letters(yr, y_at, y_cg);
                const u32 vx = x_at | x_cg, vy = y_at | y_cg;
                // the complement: A <-> T is ^ 0x15, C <-> G is ^ 0x04 (the case bit stays); any other byte becomes N
                const u32 y = ((yr ^ ((y_at >> 7) * 0x15u) ^ ((y_cg >> 7) * 0x04u)) & spread(vy)) | (('N' * ONES) & ~spread(vy));
                const u32 same = zero_bytes((x ^ y) & 0xDFDFDFDFu);
                // a byte of ones per position: covered by X, by Y, by both; valid in X, in Y, in both; the same letter
                const u32 cxM = cover(i0, 0, (int)x1), cyM = cover(i0, (int)y0, (int)I), ovM = cxM & cyM;
                const u32 bxM = spread(vx), byM = spread(vy), bothM = bxM & byM, smM = spread(same);
                // the quality rule, per byte: every candidate q capped (so phred_base + q stays inside its byte), qy > qx, qx == qy
                u32 sumW = 0, difW = 0, qxW = 0, qyW = 0, takeM = 0, tieM = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int ex = (int)((qxw >> (8 * k)) & 0xFFu) - (int)a.phred_base, ey = (int)((qyw >> (8 * k)) & 0xFFu) - (int)a.phred_base;
                    const u32 qx = (u32)(ex > 0 ? ex : 0), qy = (u32)(ey > 0 ? ey : 0);
                    const u32 hi = qx > qy ? qx : qy, lo = qx > qy ? qy : qx;
                    auto capped = [&a](u32 q) { return q < a.q_cap ? q : a.q_cap; };
                    sumW |= capped(qx + qy) << (8 * k);
                    difW |= capped(hi - lo) << (8 * k);
                    qxW |= capped(qx) << (8 * k);
                    qyW |= capped(qy) << (8 * k);
                    takeM |= ((u32)((int)(qx - qy) >> 31) & 0xFFu) << (8 * k);
                    tieM |= ((u32)((int)((qx ^ qy) - 1u) >> 31) & 0xFFu) << (8 * k);
                }
                // AGREE: X's byte, qx + qy.  DIS: the better one, a tie goes to mate 1, |qx - qy|.  ONE: the valid one.  NONE: N, 0.
                // One mate alone: its byte, its quality byte.
                const u32 disM = ovM & bothM & ~smM, noneM = ovM & ~(bxM | byM);
                const u32 fromY = (ovM & ((bothM & ~smM & takeM) | (~bothM & byM))) | (~ovM & ~cxM);
                const u32 wb = (((y & fromY) | (x & ~fromY)) & ~noneM) | (('N' * ONES) & noneM);
                const u32 qW = (bothM & ((smM & sumW) | (~smM & difW))) | (~bothM & ((bxM & qxW) | (byM & qyW)));
                const u32 wq = (ovM & (a.phred_base * ONES + qW)) | (~ovM & ((cxM & qxw) | (~cxM & qyw)));
                cnt_a += (u32)__popc(disM & ONES) + ((u32)__popc(disM & takeM & ONES) << 12) + ((u32)__popc(noneM & ONES) << 24);
                cnt_b += (u32)__popc(disM & tieM & ONES) + ((u32)__popc(ovM & (bxM ^ byM) & ONES) << 12);
                if (OUT) store4(ob, i0, I, wb, true);
                if (oq) store4(oq, i0, I, wq, oq_dword);
            }
            cnt = wave_sum((u64)(cnt_a & 0xFFFFFFu) | ((u64)cnt_b << 24) | ((u64)(cnt_a >> 24) << 48));
        }
        if (a.rows && lane < KMX_RM_WORDS) {
            static_assert(KMX_RM_LEN == 0u && KMX_RM_OVERLAP == 1u && KMX_RM_TAKEN == 2u && KMX_RM_INVALID == 3u && KMX_RM_WORDS == 4u,
                          "the order of a row's words");
            const u64 dis = cnt & 0xFFFu, taken = (cnt >> 12) & 0xFFFu, tie = (cnt >> 24) & 0xFFFu, one = (cnt >> 36) & 0xFFFu, none = cnt >> 48;
            const bool b0 = (lane & 1u) != 0u, b1 = (lane & 2u) != 0u;
            const u64 w01 = b0 ? (u64)n_ov | (dis << 32) : (u64)I, w23 = b0 ? one | (none << 32) : taken | (tie << 32);
            a.rows[r * KMX_RM_WORDS + lane] = b1 ? w23 : w01;
        }
    }
}

// the plan: the partial sums (merged pairs, merged bases) of every block and six words for the host
size_t reads_merge_bytes(u64 n_reads) { return plan_bytes(n_reads, 6u); }

hipError_t launch_reads_merge_count(const ReadsPairMerge& a, void* area, unsigned long long* h_pinned, u64* h_out, hipStream_t st) {
    const Plan p = plan_at(area, a.n_reads);
    hipLaunchKernelGGL(reads_merge_plan_count_kernel, dim3((unsigned)p.n_blocks), dim3(CT), 0, st, a, p.partial, p.n_blocks, p.tail);
    return plan_totals(p, 6u, h_pinned, h_out, st);
}

hipError_t launch_reads_merge_emit(const ReadsPairMerge& a, void* area, int n_cu, hipStream_t st) {
    const Plan p = plan_at(area, a.n_reads);
    if (a.out_offsets) hipLaunchKernelGGL(reads_merge_plan_write_kernel, dim3((unsigned)p.n_blocks), dim3(CT), 0, st, a, p.partial, p.n_blocks, p.tail);
    const dim3 grid(wave_per_read_grid(a.n_reads, n_cu));
    if (a.quals1) {
        if (a.out_bases) hipLaunchKernelGGL((reads_merge_kernel<true, true>), grid, dim3(WPR_THREADS), 0, st, a);
        else hipLaunchKernelGGL((reads_merge_kernel<true, false>), grid, dim3(WPR_THREADS), 0, st, a);
    } else {
        if (a.out_bases) hipLaunchKernelGGL((reads_merge_kernel<false, true>), grid, dim3(WPR_THREADS), 0, st, a);
        else hipLaunchKernelGGL((reads_merge_kernel<false, false>), grid, dim3(WPR_THREADS), 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace kmx
