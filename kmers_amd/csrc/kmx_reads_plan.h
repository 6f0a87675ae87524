// kmx_reads_plan.h -- the plan of a read-preparation call that produces a batch (kmx_reads_edit.hip, kmx_reads_merge.hip): its
// blocks, its place in the work area, the body of its count kernel, and the two scans with the read-back behind it.  On top of
// kmx_reads_common.h and of the count family's block sum, scan kernel and read_back (kmx_count_common.h).  Internal linkage.
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

}  // namespace

}  // namespace kmx
