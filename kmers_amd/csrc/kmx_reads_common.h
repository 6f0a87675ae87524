// kmx_reads_common.h -- what the four kmx_reads_*.hip units share: the span of a read (the one place that states the rules "an
// offsets pair that descends: 0" and "2^31 bases or more: 0"), "is one of ACGTacgt" and the launch shape of the wave-per-read
// kernels.  The plan of the two units that produce a batch is kmx_reads_plan.h, on top of this header: it stands on
// kmx_count_common.h, whose kernels go into every object that includes it, so the units without a plan stay clear of it.
#pragma once
#include "kmx_device.h"
#include "kmx_launch.h"

namespace kmx {

namespace {

// the bases between two offsets (kmx.h, THE SPAN OF A READ): 0 for a pair that descends, 0 for 2^31 bases or more
__host__ __device__ __forceinline__ u32 span_len(u64 b, u64 e) {
    const u64 n = e >= b ? e - b : 0u;
    return n >= (1ull << 31) ? 0u : (u32)n;
}

// the length of read r and, in `off`, where its first byte lies in d_bases (offsets == nullptr: uniform reads of read_len bases)
__host__ __device__ __forceinline__ u32 read_span(const u64* offsets, u32 read_len, u64 r, u64& off) {
    u64 b = 0u, e = read_len;
    if (offsets) {
        b = off = offsets[r];
        e = offsets[r + 1u];
    } else {
        off = r * (u64)read_len;
    }
    return span_len(b, e);
}

__host__ __device__ __forceinline__ bool is_acgt(u32 b) {
    const u32 u = b & 0xDFu;
    return u == 'A' || u == 'C' || u == 'G' || u == 'T';
}

// a wave per read: the launch shape
constexpr u32 WPR_THREADS = 256;                 // threads per block
constexpr u32 WPR_WAVES = WPR_THREADS / 64u;     // reads a block has in flight
constexpr u32 WPR_BLOCKS_PER_CU = 8;             // 8 waves per SIMD
// a wave per read up to four rounds of resident blocks; beyond that the waves stride over the reads
unsigned wave_per_read_grid(u64 n_reads, int n_cu) {
    const u64 want = (n_reads + WPR_WAVES - 1u) / WPR_WAVES;
    const u64 cap = (u64)(n_cu > 0 ? n_cu : 256) * WPR_BLOCKS_PER_CU * 4u;
    return (unsigned)(want < cap ? want : cap);
}

}  // namespace

}  // namespace kmx
