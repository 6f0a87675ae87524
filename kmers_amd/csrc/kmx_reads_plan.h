// kmx_reads_plan.h -- the plan of a read-preparation call that produces a batch or an image (kmx_reads_edit.hip, kmx_reads_merge.hip,
// kmx_fastx_format.hip): its blocks, its place in the work area, the body of its count kernel, and the two scans with the read-back
// behind it; and what the two copies built around the output share (kmx_reads_edit.hip, kmx_fastx_format.hip): the block's search
// and a piece's bytes out of aligned dword loads.  On top of kmx_reads_common.h and of the count family's block sum, scan kernel
// and read_back (kmx_count_common.h).  Internal linkage.
#pragma once
#include "kmx_count_common.h"
#include "kmx_reads_common.h"

namespace kmx {

namespace {

// A thread plans RPT consecutive rows, a block ROWS.  The plan lies in 2 n_blocks + n_tail words of the work area: partial[b] = the
// kept rows of block b, partial[n_blocks + b] = their bytes, then the tail: the two totals and what else the host wants to see.
constexpr u32 RPT = 8;
constexpr u32 ROWS = CT * RPT;
struct Plan {
    u64* partial;
    u64 n_blocks;
    u64* tail;
};
u64 plan_blocks(u64 n_rows) { return ceil_div(n_rows, (u64)ROWS); }
size_t plan_bytes(u64 n_rows, u32 n_tail) { return align256(8u * (2u * plan_blocks(n_rows) + n_tail)); }
Plan plan_at(void* area, u64 n_rows) {
    u64* const partial = static_cast<u64*>(area);
    const u64 nb = plan_blocks(n_rows);
    return Plan{partial, nb, partial + 2u * nb};
}

struct PlanRow {
    bool kept;
    u64 len;   // 0 for a row that is not kept
};

// The body of a plan's count kernel (CT threads, plan_blocks(n_rows) blocks): the block's sums of row(i) -> PlanRow into `partial`;
// thread 0 of block 0 then calls first_last(), which writes the batch's first and last offsets into the tail from word 2 on.
template <class Row, class FirstLast>
__device__ __forceinline__ void plan_count(u64 n_rows, u64* partial, u64 n_blocks, Row row, FirstLast first_last) {
    __shared__ u64 sh[CT / 64];
    const u64 i0 = (u64)blockIdx.x * ROWS + (u64)threadIdx.x * RPT;
    u64 n = 0, bytes = 0;
#pragma unroll
    for (u32 j = 0; j < RPT; ++j) {
        if (i0 + j < n_rows) {
            const PlanRow c = row(i0 + j);
            n += c.kept ? 1u : 0u;
            bytes += c.len;
        }
    }
    const u64 tn = block_sum(n, sh);
    const u64 tb = block_sum(bytes, sh);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = tn;
        partial[n_blocks + blockIdx.x] = tb;
        if (blockIdx.x == 0) first_last();
    }
}

// behind the count kernel: one block scans each array of partial sums (totals into tail[0], tail[1]) and the tail's n_tail words
// come back to the host.  Synchronous: one host round trip.
hipError_t plan_totals(const Plan& p, u32 n_tail, unsigned long long* h_pinned, u64* h_out, hipStream_t st) {
    hipLaunchKernelGGL(scan_single_kernel, dim3(1), dim3(CT), 0, st, p.partial, p.n_blocks, p.tail);
    hipLaunchKernelGGL(scan_single_kernel, dim3(1), dim3(CT), 0, st, p.partial + p.n_blocks, p.n_blocks, p.tail + 1);
    return read_back(h_pinned, p.tail, n_tail, h_out, st);
}

// ---- the copy built around the output (kmx_reads_edit.hip, kmx_fastx_format.hip): the block's search, and a piece's bytes
// out of aligned dword loads ----
// The search of a block for the output read that holds byte p: off[lo] <= p < off[hi] throughout (off[0] = 0, off[n_out] = n_bases > p,
// offsets ascend).  A round: thread t probes off[at(t)] where at(t) < hi; the probes ascend with t, so those at or below p are the
// first c of them, and take(c) narrows the range to one step: 256-fold.
struct BlockSearch {
    u64 lo, hi;
    __host__ __device__ __forceinline__ bool done() const { return hi - lo <= 1u; }
    __host__ __device__ __forceinline__ u64 step() const { return ceil_div(hi - lo, (u64)CT); }
    __host__ __device__ __forceinline__ u64 at(u32 t) const { return lo + ((u64)t + 1u) * step(); }
    __host__ __device__ __forceinline__ void take(u64 c) {
        const u64 st = step();
        lo += c * st;
        hi = lo + st < hi ? lo + st : hi;
    }
};

// The n bytes at bases + s (n in 1 .. 16) are to lie at byte b0 of a piece (b0 + n <= 16).  Five aligned dwords cover the piece's 16
// bytes in the source's address space; load_words loads those that hold a byte of [s, s + n) and no other, merge_words lines them up
// with the piece (a funnel shift by the source's byte phase) and ors the n bytes into d.  `phase` = the address of `bases` mod 4:
// dwords are aligned in memory, not in the batch.  Positions are counted from bases - phase - 16, a dword boundary: the piece's
// byte 0 may line up with a byte up to 15 before the batch.
__host__ __device__ __forceinline__ void load_words(u32 (&w)[5], const uint8_t* bases, u32 phase, u64 s, u32 n, u32 b0) {
    const u64 sp = s + phase + 16u, base = (sp - b0) & ~3ull, s_end = sp + n;
    const uint8_t* const origin = bases - phase - 16;
#pragma unroll
    for (u32 i = 0; i < 5; ++i) {
        const u64 wa = base + 4u * i;
        w[i] = (wa + 4u > sp && wa < s_end) ? *reinterpret_cast<const u32*>(origin + wa) : 0u;
    }
}

__host__ __device__ __forceinline__ void merge_words(u32 (&d)[4], const u32 (&w)[5], u32 phase, u64 s, u32 n, u32 b0) {
    const u32 sh = (u32)((s + phase + 16u - b0) & 3u) * 8u;
    const u32 m16 = ((1u << n) - 1u) << b0;   // the piece's bytes this read fills
#pragma unroll
    for (u32 i = 0; i < 4; ++i) {
        const u32 v = (u32)((((u64)w[i + 1] << 32) | w[i]) >> sh);
        const u32 nib = (m16 >> (4u * i)) & 15u;
        const u32 m = ((nib | (nib << 7) | (nib << 14) | (nib << 21)) & 0x01010101u) * 0xFFu;   // a byte of ones per bit
        d[i] |= v & m;
    }
}

// the piece's n bytes from byte `first` on go to `piece`: one 16-byte store, or -- the batch's first or last piece -- byte by byte
__host__ __device__ __forceinline__ void store_piece(uint8_t* piece, const u32 (&d)[4], u32 first, u32 n) {
    if (n == 16u) {   // (first == 0: piece is 16-byte aligned)
        *reinterpret_cast<uint4*>(piece) = make_uint4(d[0], d[1], d[2], d[3]);
    } else {
#pragma unroll
        for (u32 b = 0; b < 16; ++b)
            if (b >= first && b - first < n) piece[b - first] = (uint8_t)(d[b >> 2] >> (8u * (b & 3u)));
    }
}

}  // namespace

}  // namespace kmx
