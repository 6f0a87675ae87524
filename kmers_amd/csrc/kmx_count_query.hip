// kmx_count_query.hip -- what is done WITH a count table (kmx_count_canonical(2) / kmx_count_merge(2): keys ascending and distinct,
// one u64 count per key): kmx_count_lookup(2) / kmx_count_lookup_reads(2), kmx_count_spectrum, kmx_count_filter(2).
//
// Lookup.  A batch of unrelated queries against a sorted array: nothing coalesces, every query is a chain of dependent loads, and
// what hides the chain is the number of chains in flight.  Two routes, one kernel:
//   directory  dir[j] = index of the first key whose top p bits (counted down from bit 2k, as the counter's MSD partition counts
//              them) are >= j, j = 0 .. 2^p; p from n so that a bin holds about LINE keys when keys are evenly spread.  Built per
//              call by one streaming pass over the keys (kmx_count_dir.h: bin_of, dir_build_kernel, shared with the adjacency).
//              Per query: dir[j], dir[j + 1], then the search confined to that bin.
//   plain      the same search over [0, n): few queries against a large table (the pass over the keys would cost more than it
//              saves), a directory above the work buffer's cap, a table of 2^32 entries or more (directory entries are 4 bytes).
// The search is correct for a bin of any size (all n keys in one bin, empty bins): binary steps while the range is longer than LINE
// keys, then the LINE keys of the range are loaded at once (independent loads, one latency) and compared.  QPL queries per lane run
// in lockstep, so every step issues QPL independent loads.  Vector loads and stores only; no LDS, no atomics, no scratch.
// A table that is not sorted gives wrong answers, never a wild access: directory entries are clamped to n before they are used.
//
// Spectrum.  Bins below SPEC_LDS in block-private LDS words (u32: a block sees fewer than 2^32 entries), the rest -- rare in a real
// table, where small counts dominate -- straight to the output with device atomics; count == 1 (most rows of a real table) and the
// last, collecting bin (most rows of a deep table with few bins) are tallied per thread and added once per wave.  The block's bins are added to the output with one device atomic per non-empty bin.
//
// Filter.  A mark byte per entry, then the counters' compaction, all of it in kmx_count_common.h: keep_count_kernel, the block
// scans, and the wave-ballot copy of the marked entries (compact_write_kernel<W, 1>: a table's counts are plain u64).
#include "kmx_count_dir.h"

namespace kmx {

namespace {

constexpr u32 QPL = 4;           // queries per lane, in lockstep
constexpr u32 SPEC_LDS = 4096;   // spectrum bins held in LDS per block (16 KiB)
constexpr u32 SPEC_IPT = 16;     // entries per thread and grid step of the spectrum

// ---------------------------------------------------------------- the lookup
// out[i] = count of query[i] (1 with counts == nullptr), 0 if absent or the query's flag lacks KMX_WIN_VALID.  `out` may be `query`
// (one-word keys): a lane reads its own queries before it writes their answers, and nobody else's.
template <u32 W, bool DIR>
__global__ void __launch_bounds__(CT) lookup_kernel(const u64* __restrict__ keys, const u64* __restrict__ counts, u64 n, u32 k, u32 p,
                                                    const u32* __restrict__ dir, const u64* query, const uint8_t* __restrict__ qflags, u64 n_query,
                                                    u64* out) {
    using K = Key<W>;
    const u64 base = (u64)blockIdx.x * (CT * QPL) + threadIdx.x;
    K q[QPL];
    u64 lo[QPL], hi[QPL];
    bool live[QPL];
#pragma unroll
    for (u32 j = 0; j < QPL; ++j) {
        const u64 i = base + (u64)j * CT;
        live[j] = i < n_query;
        q[j] = K::load(query, live[j] ? i : 0u);
        if (live[j] && qflags != nullptr) live[j] = (qflags[i] & KMX_WIN_VALID) != 0u;
        if (q[j].outside(k)) live[j] = false;
    }
#pragma unroll
    for (u32 j = 0; j < QPL; ++j) {
        lo[j] = hi[j] = 0u;
        if (!live[j]) continue;
        if (DIR) {
            const u64 b = bin_of<W>(q[j], k, p);
            const u64 a0 = dir[b], a1 = dir[b + 1u];
            lo[j] = a0 < n ? a0 : n;
            hi[j] = a1 < n ? a1 : n;
            if (hi[j] < lo[j]) hi[j] = lo[j];
        } else {
            hi[j] = n;
        }
    }
    // binary steps while some range is longer than LINE keys; q, if the table holds it, stays inside [lo, hi): keys[mid] <= q keeps
    // [mid, hi), q < keys[mid] keeps [lo, mid) (lo < mid < hi, so every step shortens the range)
    for (;;) {
        bool any = false;
#pragma unroll
        for (u32 j = 0; j < QPL; ++j) any |= hi[j] - lo[j] > LINE;
        if (!any) break;
        K m[QPL];
        u64 mid[QPL];
#pragma unroll
        for (u32 j = 0; j < QPL; ++j) {
            mid[j] = lo[j] + ((hi[j] - lo[j]) >> 1);
            m[j] = q[j];
            if (hi[j] - lo[j] > LINE) m[j] = K::load(keys, mid[j]);
        }
#pragma unroll
        for (u32 j = 0; j < QPL; ++j) {
            if (hi[j] - lo[j] > LINE) {
                if (q[j].less(m[j])) hi[j] = mid[j];
                else lo[j] = mid[j];
            }
        }
    }
    // at most LINE keys are left: load them all, the equal one (keys are distinct) is the answer
    u64 hit[QPL];
#pragma unroll
    for (u32 j = 0; j < QPL; ++j) {
        hit[j] = ~0ull;
#pragma unroll
        for (u32 s = 0; s < LINE; ++s) {
            const u64 i = lo[j] + s;
            if (i < hi[j] && K::load(keys, i).equal(q[j])) hit[j] = i;
        }
    }
#pragma unroll
    for (u32 j = 0; j < QPL; ++j) {
        const u64 i = base + (u64)j * CT;
        if (i >= n_query) continue;
        u64 v = 0u;
        if (hit[j] != ~0ull) v = counts != nullptr ? counts[hit[j]] : 1u;
        out[i] = v;
    }
}

// ---------------------------------------------------------------- the spectrum
__global__ void __launch_bounds__(CT) spectrum_kernel(const u64* __restrict__ counts, u64 n, u64 n_bins, unsigned long long* __restrict__ spectrum) {
    __shared__ u32 bins[SPEC_LDS];
    for (u32 b = threadIdx.x; b < SPEC_LDS; b += CT) bins[b] = 0u;
    __syncthreads();
    const u64 top = n_bins - 1u;
    u32 ones = 0, tops = 0;
    for (u64 i0 = (u64)blockIdx.x * (CT * SPEC_IPT) + threadIdx.x; i0 < n; i0 += (u64)gridDim.x * (CT * SPEC_IPT)) {
        u64 c[SPEC_IPT];
#pragma unroll
        for (u32 j = 0; j < SPEC_IPT; ++j) {
            const u64 i = i0 + (u64)j * CT;
            c[j] = i < n ? counts[i] : 0u;
        }
#pragma unroll
        for (u32 j = 0; j < SPEC_IPT; ++j) {
            if (i0 + (u64)j * CT >= n) continue;
            const u64 b = c[j] < top ? c[j] : top;
            if (b == top) tops += 1u;   // (the collecting bin: most rows of a deep table with few bins; n_bins == 2: the singletons too)
            else if (b == 1u) ones += 1u;
            else if (b < SPEC_LDS) atomicAdd(&bins[b], 1u);
            else atomicAdd(&spectrum[b], 1ull);
        }
    }
    for (u32 o = 32; o > 0; o >>= 1) {
        ones += __shfl_xor(ones, o);
        tops += __shfl_xor(tops, o);
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (ones != 0u) atomicAdd(&bins[1], ones);
        if (tops != 0u) {
            if (top < SPEC_LDS) atomicAdd(&bins[top], tops);
            else atomicAdd(&spectrum[top], (unsigned long long)tops);
        }
    }
    __syncthreads();
    for (u32 b = threadIdx.x; b < SPEC_LDS; b += CT) {
        const u32 v = bins[b];
        if (v != 0u) atomicAdd(&spectrum[b], (unsigned long long)v);   // (b < n_bins: only clamped values were counted)
    }
}

// ---------------------------------------------------------------- the filter
// keep[i] = min <= counts[i] <= max over the whole padded range (the compaction reads whole CHUNKs)
__global__ void __launch_bounds__(CT) filter_mark_kernel(const u64* __restrict__ counts, u64 n, u64 n_pad, u64 mn, u64 mx, uint8_t* __restrict__ keep) {
    const u64 i = (u64)blockIdx.x * CT + threadIdx.x;
    if (i >= n_pad) return;
    const bool in = i < n;
    const u64 c = in ? counts[i] : 0u;
    keep[i] = in && c >= mn && c <= mx ? 1u : 0u;
}

u64 filter_pad(u64 n) { return ceil_div(n, CHUNK) * CHUNK; }

}  // namespace

// ---------------------------------------------------------------- host side
// The directory for a table of n keys of 2k bits: *p_out prefix bits, 4 * (2^p + 1) bytes; 0 = no directory for such a table.
size_t count_lookup_dir_bytes(u64 n, u32 k, u32* p_out) {
    *p_out = 0;
    if (n == 0 || n >= (1ull << 32)) return 0;
    u32 p = 0;
    while (p < DIR_MAX_BITS && p < 2u * k && (n >> p) > LINE) ++p;   // n / 2^p <= LINE, or as many bits as there are
    *p_out = p;
    return align256(4u * ((1ull << p) + 1u));
}

// Is the directory worth its pass over the keys?  Building it streams 8 * words * n bytes; a query it serves touches one line of
// the directory and one or two of its bin instead of the lines of a whole search's last steps that no cache holds: about four
// 128-byte lines, 512 bytes, saved per query.
bool count_lookup_wants_dir(u64 n, u64 n_query, u32 words) { return n > LINE && n_query >= (u64)words * n / 64u; }

hipError_t launch_count_lookup(u32 words, const u64* keys, const u64* counts, u64 n, u32 k, const u64* query, const uint8_t* qflags, u64 n_query,
                               u64* out, void* dir_area, u32 p, hipStream_t st) {
    u32* dir = static_cast<u32*>(dir_area);
    const unsigned nb = (unsigned)ceil_div(n + 1u, CT), nq = (unsigned)ceil_div(n_query, (u64)CT * QPL);
    with_width(words, [&](auto w) {
        constexpr u32 W = decltype(w)::value;
        if (dir) hipLaunchKernelGGL(dir_build_kernel<W>, dim3(nb), dim3(CT), 0, st, keys, n, k, p, dir);
        if (dir) hipLaunchKernelGGL((lookup_kernel<W, true>), dim3(nq), dim3(CT), 0, st, keys, counts, n, k, p, dir, query, qflags, n_query, out);
        else hipLaunchKernelGGL((lookup_kernel<W, false>), dim3(nq), dim3(CT), 0, st, keys, counts, n, k, p, dir, query, qflags, n_query, out);
    });
    return hipGetLastError();
}

hipError_t launch_count_spectrum(const u64* counts, u64 n, u64 n_bins, u64* spectrum, int n_cu, hipStream_t st) {
    u64 nb = ceil_div(n, (u64)CT * SPEC_IPT);
    const u64 cap = (u64)(n_cu > 0 ? n_cu : 256) * 8u;
    if (nb > cap) nb = cap;
    hipLaunchKernelGGL(spectrum_kernel, dim3((unsigned)nb), dim3(CT), 0, st, counts, n, n_bins, reinterpret_cast<unsigned long long*>(spectrum));
    return hipGetLastError();
}

// the filter's working set: a mark byte per entry (whole CHUNKs) and a partial sum per CHUNK
size_t count_filter_bytes(u64 n) { return align256(filter_pad(n)) + align256(8u * (ceil_div(n, CHUNK) + 2u)); }

// marks and counts the entries of [min, max]; synchronous (one host round trip: how many there are)
hipError_t launch_count_filter_mark(const u64* counts, u64 n, u64 mn, u64 mx, void* area, unsigned long long* h_pinned, u64* h_out, hipStream_t st) {
    uint8_t* keep = static_cast<uint8_t*>(area);
    u64* partial = reinterpret_cast<u64*>(static_cast<char*>(area) + align256(filter_pad(n)));
    const u64 nb = ceil_div(n, CHUNK);
    hipLaunchKernelGGL(filter_mark_kernel, dim3((unsigned)ceil_div(filter_pad(n), CT)), dim3(CT), 0, st, counts, n, filter_pad(n), mn, mx, keep);
    hipLaunchKernelGGL(keep_count_kernel, dim3((unsigned)nb), dim3(CT), 0, st, keep, partial);
    hipLaunchKernelGGL(scan_single_kernel, dim3(1), dim3(CT), 0, st, partial, nb, partial + nb);
    return read_back(h_pinned, partial + nb, 1u, h_out, st);
}

hipError_t launch_count_filter_emit(u32 words, const u64* keys, const u64* counts, u64 n, const void* area, u64* out_k, u64* out_c, hipStream_t st) {
    const uint8_t* keep = static_cast<const uint8_t*>(area);
    const u64* partial = reinterpret_cast<const u64*>(static_cast<const char*>(area) + align256(filter_pad(n)));
    const unsigned nb = (unsigned)ceil_div(n, CHUNK);
    if (words == 1u) hipLaunchKernelGGL((compact_write_kernel<1, 1>), dim3(nb), dim3(CT), 0, st, keep, partial, keys, counts, out_k, out_c);
    else hipLaunchKernelGGL((compact_write_kernel<2, 1>), dim3(nb), dim3(CT), 0, st, keep, partial, keys, counts, out_k, out_c);
    return hipGetLastError();
}

}  // namespace kmx
