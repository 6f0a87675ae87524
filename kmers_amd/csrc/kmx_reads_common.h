// kmx_reads_common.h -- what the kmx_reads_*.hip units share: the span of a read (the one place that states the rules "an
// offsets pair that descends: 0" and "2^31 bases or more: 0"), "is one of ACGTacgt", the launch shape of the wave-per-read
// kernels, and the four-bytes-a-lane fetch with its byte-wise helpers (kmx_reads_merge.hip, kmx_reads_dedup.hip).
// The plan of the two units that produce a batch is kmx_reads_plan.h, on top of this header: it stands on kmx_count_common.h, whose
// kernels go into every object that includes it, so the units that need none of it stay clear of it.
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

// ---- four bytes of a read a lane (the merge and the duplicate kernels): the fetch, and SWAR on the bytes of a dword ----
constexpr u32 ONES = 0x01010101u, HIGH = 0x80808080u;

// The four bytes base[at .. at + 3] (byte k in bits 8 k ..; `at` may be negative) out of the two aligned dwords that hold them, for
// base[0 .. n), n >= 1.  Positions count on the dword grid of `base`, g = at + (the address of base mod 4), and the two dword
// positions are clamped to the first and the last dword that hold a byte of base[0 .. n): no other dword is loaded, and no branch
// is taken.  A byte that lies outside base[0 .. n) comes back as some byte of those dwords: the caller does not use it.
__device__ __forceinline__ u32 load4(const uint8_t* base, int at, u32 n) {
    const int ph = (int)(reinterpret_cast<uintptr_t>(base) & 3u);
    const int g = at + ph, g0 = g & ~3, last = (ph + (int)n - 1) & ~3;
    auto clamp = [last](int v) { return v < 0 ? 0 : v > last ? last : v; };
    const uint8_t* const origin = base - ph;
    const u32 w0 = *reinterpret_cast<const u32*>(origin + clamp(g0)), w1 = *reinterpret_cast<const u32*>(origin + clamp(g0 + 4));
    return __builtin_amdgcn_alignbyte(w1, w0, (u32)(g & 3));   // bytes (g & 3) .. + 3 of w1:w0
}

// bit 7 of every byte of z that is zero (exact: no carry crosses a byte)
__device__ __forceinline__ u32 zero_bytes(u32 z) { return ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & HIGH; }
// bit 7 of every byte of w that is A / T (at) or C / G (cg), either case
__device__ __forceinline__ void letters(u32 w, u32& at, u32& cg) {
    const u32 u = w & 0xDFDFDFDFu;
    at = zero_bytes(u ^ ('A' * ONES)) | zero_bytes(u ^ ('T' * ONES));
    cg = zero_bytes(u ^ ('C' * ONES)) | zero_bytes(u ^ ('G' * ONES));
}
// a byte of ones for every bit 7 set in m
__device__ __forceinline__ u32 spread(u32 m) { return (m >> 7) * 0xFFu; }

// a wave per read: the launch shape
constexpr u32 WPR_THREADS = 256;                // threads per block
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
