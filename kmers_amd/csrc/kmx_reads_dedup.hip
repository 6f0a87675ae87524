// kmx_reads_dedup.hip -- duplicate reads and read pairs: kmx_reads_dedup.  kmx.h has the contract (codes, fingerprint, key, rank, the
// decision, the words of a row); DESIGN 4.6.18 has the reasoning and the figures.
//
// Hash, sort, verify.  Four steps, every one a kernel boundary after the other; no block waits for another.
//   key     A WAVE PER ITEM.  A lane owns positions [4 (64 s + lane), + 4) of step s of a read: its four bytes out of two clamped aligned
//           dwords (load4, kmx_reads_common.h), four codes by SWAR, one fmix term; the terms are summed over the wave.  The fingerprint
//           is a sum of position-keyed terms, so it does not depend on where the read lies on the dword grid.  Under KMX_DD_STRAND a
//           single read is walked a second time from the back with the complement (the same cache lines); a pair needs no reverse
//           complement, its other strand is its mates exchanged.  Lane 0 writes one 16-byte record {lo = (2^32 - 1 - s) << 32 | r,
//           hi = Hc} in the slot layout of two-word keys, its flag byte, the byte with OTHER (bit 0) and F_a == F_b (bit 1), and COUNT = 0.
//   sort    The records are two-word keys, ordered high word first: by key, then by rank, then by index.  The two-word counter sorts
//           them (launch_count_sort with k = 64, launch_count_emit): all records are distinct, so the table it leaves IS the sorted
//           records.  No sort of its own.
//   groups  A sorted position is a head where its high word differs from its predecessor's.  Block counts of heads, the family's
//           one-block scan, and a write pass: every sorted position gets the ordinal of its group and every group the item index of
//           its head (the two arrays lie where the sort left its counts, which nobody reads).
//   verify  A WAVE PER SORTED POSITION.  A head writes its row.  Any other item is compared with its head, four codes a lane per step
//           with the fetch of the key kernel, one ballot per comparison; the orientation follows from the two OTHER bits unless F_a
//           == F_b for either item, where both are tried.  Lane 0 writes the row and the keep byte and adds to the head's COUNT; every
//           add is + 1, so the largest value an add leaves behind is the largest COUNT.  The four summary words are kept per wave,
//           written once per wave and folded by one block behind the kernel.  Integer atomics only: repeated calls give identical bytes.
// The wave-per-item kernels use no LDS and no scratch and stay within 64 VGPRs (eight waves per SIMD, the family's convention).
#include "kmx_count_common.h"
#include "kmx_reads_common.h"

namespace kmx {

namespace {

constexpr u64 DD_G = 0x9E3779B97F4A7C15ull;
constexpr u32 DD_OTHER = 1u, DD_AMBIGUOUS = 2u;   // the bits of an item's byte: F_b < F_a, F_a == F_b (both only under KMX_DD_STRAND)

__device__ __forceinline__ u64 pair_hash(u64 x, u64 y) { return fmix64(fmix64(x + DD_G) + y); }

// the codes of four bytes, one per byte: 0, 1, 2, 3 for A, C, G, T in either case, 4 for any other byte; comp: of the complement
__device__ __forceinline__ u32 codes4(u32 w, bool comp) {
    u32 at, cg;
    letters(w, at, cg);
    const u32 ok = spread(at | cg);
    const u32 x = (w >> 1) & (3u * ONES);   // A 0, C 1, G 3, T 2
    u32 c = x ^ ((x >> 1) & ONES);          // A 0, C 1, G 2, T 3
    if (comp) c ^= 3u * ONES;
    return (c & ok) | ((4u * ONES) & ~ok);
}
// a byte of ones for every position q0 + k < L (q0 < L)
__device__ __forceinline__ u32 inside(u32 q0, u32 L) {
    const u32 n = L - q0;
    return n >= 4u ? ~0u : ~(~0u << (8u * n));
}
// the codes of positions q0 .. q0 + 3 (q0 < L, a multiple of 4) of the read base[0 .. L) or, rc, of its reverse complement: position
// q of the reverse complement is the complement of byte L - 1 - q.  The bytes of positions at or past L are the caller's to mask.
__device__ __forceinline__ u32 codes_at(const uint8_t* base, u32 L, u32 q0, bool rc) {
    return rc ? codes4(__builtin_bswap32(load4(base, (int)L - 4 - (int)q0, L)), true) : codes4(load4(base, (int)q0, L), false);
}

// H of the read or of its reverse complement (kmx.h), the same in every lane; every lane of the wave enters
__device__ __forceinline__ u64 read_hash(const uint8_t* base, u32 L, bool rc, u32 lane) {
    u64 sum = 0;
    for (u32 q0 = 4u * lane; q0 < L; q0 += 256u) {
        const u32 m = inside(q0, L);
        const u32 c = (codes_at(base, L, q0, rc) & m) | ((0xFu * ONES) & ~m);
        const u32 v = (c & 0xFu) | ((c >> 4) & 0xF0u) | ((c >> 8) & 0xF00u) | ((c >> 12) & 0xF000u);
        sum += fmix64((((u64)(q0 >> 2) << 16) | v) + DD_G);
    }
    return fmix64(wave_sum(sum) ^ ((u64)L * DD_G));
}

// x[0 .. Lx) and y[0 .. Ly), or with rc the reverse complement of y, are the same code sequence; every lane of the wave enters
__device__ __forceinline__ bool reads_equal(const uint8_t* x, u32 Lx, const uint8_t* y, u32 Ly, bool rc, u32 lane) {
    if (Lx != Ly) return false;
    u32 diff = 0;
    for (u32 q0 = 4u * lane; q0 < Lx; q0 += 256u) diff |= (codes_at(x, Lx, q0, false) ^ codes_at(y, Lx, q0, rc)) & inside(q0, Lx);
    return __ballot(diff != 0u) == 0ull;
}

// where the reads of item r lie
struct Item {
    const uint8_t *b1, *b2;
    u32 L1, L2;
};
// load4 counts dword positions in an int: phase + length - 1 must stay below 2^31, so the last four lengths below 2^31 are 0 as well
__device__ __forceinline__ u32 fetchable(u32 L) { return L > 0x7FFFFFFBu ? 0u : L; }
__device__ __forceinline__ Item item_of(const ReadsDedup& a, u64 r) {
    Item it{a.bases1, a.bases2, 0u, 0u};
    u64 off = 0;
    it.L1 = fetchable(read_span(a.offsets1, a.read_len1, r, off));
    it.b1 += off;
    if (a.pairs) {
        it.L2 = fetchable(read_span(a.offsets2, a.read_len2, r, off));
        it.b2 += off;
    }
    return it;
}

__global__ void __launch_bounds__(WPR_THREADS) reads_dedup_key_kernel(const ReadsDedup a, u64* __restrict__ rec, uint8_t* __restrict__ valid,
                                                                      uint8_t* __restrict__ other) {
    const u32 lane = threadIdx.x & 63u;
    const u32 wv = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 stride = (u64)gridDim.x * WPR_WAVES;
    const u32 sh = 64u - a.hash_bits;
    for (u64 r = (u64)blockIdx.x * WPR_WAVES + wv; r < a.n_reads; r += stride) {
        const Item it = item_of(a, r);
        const u64 h1 = read_hash(it.b1, it.L1, false, lane);
        u64 fa = h1, fb = h1;
        if (a.pairs) {
            const u64 h2 = read_hash(it.b2, it.L2, false, lane);
            fa = pair_hash(h1, h2);
            fb = pair_hash(h2, h1);
        } else if (a.strand) {
            fb = read_hash(it.b1, it.L1, true, lane);
        }
        fa >>= sh;
        fb = a.strand ? fb >> sh : fa;
        if (lane == 0u) {
            u64 s = a.score ? a.score[r * a.score_stride] : 0u;
            s = s < 0xFFFFFFFFull ? s : 0xFFFFFFFFull;
            Key<2>::store(rec, r, Key<2>{((0xFFFFFFFFull - s) << 32) | r, fb < fa ? fb : fa});
            valid[r] = (uint8_t)KMX_WIN_VALID;
            other[r] = (uint8_t)(a.strand ? (fb < fa ? DD_OTHER : 0u) | (fb == fa ? DD_AMBIGUOUS : 0u) : 0u);
            a.rows[r * KMX_DD_WORDS + KMX_DD_COUNT] = 0u;
        }
    }
}

// ---------------------------------------------------------------- groups of the sorted records
__device__ __forceinline__ bool group_head(const u64* sorted, u64 i) { return i == 0u || sorted[2u * i + 1u] != sorted[2u * i - 1u]; }
__device__ __forceinline__ u64 heads_of_thread(const u64* sorted, u64 i0, u64 n) {
    u64 c = 0;
    for (u32 j = 0; j < 16; ++j)
        if (i0 + j < n && group_head(sorted, i0 + j)) ++c;
    return c;
}

__global__ void __launch_bounds__(CT) reads_dedup_head_count_kernel(const u64* __restrict__ sorted, u64 n, u64* __restrict__ partial) {
    __shared__ u64 sh[CT / 64];
    const u64 t = block_sum(heads_of_thread(sorted, (u64)blockIdx.x * MCHUNK + (u64)threadIdx.x * 16u, n), sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// group[i] = the ordinal of the group of sorted position i; head_item[g] = the item index of the head of group g
__global__ void __launch_bounds__(CT) reads_dedup_head_write_kernel(const u64* __restrict__ sorted, u64 n, const u64* __restrict__ partial,
                                                                    u32* __restrict__ group, u32* __restrict__ head_item) {
    __shared__ u64 sh[CT];
    const u64 i0 = (u64)blockIdx.x * MCHUNK + (u64)threadIdx.x * 16u;
    u64 tot;
    u64 o = partial[blockIdx.x] + block_exscan(heads_of_thread(sorted, i0, n), sh, &tot);
    for (u32 j = 0; j < 16; ++j) {
        const u64 i = i0 + j;
        if (i >= n) break;
        if (group_head(sorted, i)) head_item[o++] = (u32)sorted[2u * i];
        group[i] = (u32)(o - 1u);   // (position 0 is a head: o >= 1)
    }
}

// ---------------------------------------------------------------- the decision
// PAIRS: an item is a pair.  STRAND: KMX_DD_STRAND.
template <bool PAIRS, bool STRAND>
__global__ void __launch_bounds__(WPR_THREADS) reads_dedup_verify_kernel(const ReadsDedup a, const u64* __restrict__ sorted,
                                                                         const u32* __restrict__ group, const u32* __restrict__ head_item,
                                                                         const uint8_t* __restrict__ other, u64* __restrict__ wave_partial) {
    const u32 lane = threadIdx.x & 63u;
    const u32 wv = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 stride = (u64)gridDim.x * WPR_WAVES;
    unsigned long long kept = 0, dropped = 0, collisions = 0, largest = 0;   // lane 0's: what the wave adds to the summary
    for (u64 i = (u64)blockIdx.x * WPR_WAVES + wv; i < a.n_reads; i += stride) {
        const u64 r = sorted[2u * i] & 0xFFFFFFFFull, hc = sorted[2u * i + 1u];
        const u64 h = head_item[group[i]];
        const u32 o_r = other[r];
        bool drop = false, flipped = false;
        if (h != r) {
            // the same orientation gives both items the same F_a and F_b, so the same OTHER; the other one exchanges them, so OTHER
            // differs unless F_a == F_b.  So: as it is where OTHER agrees; the reverse complement, or the mates exchanged, where it
            // differs or either item has F_a == F_b
            const u32 o_h = other[h];
            const bool differ = ((o_r ^ o_h) & DD_OTHER) != 0u;
            const bool try_flip = STRAND && (differ || ((o_r | o_h) & DD_AMBIGUOUS) != 0u);
            const Item x = item_of(a, r), y = item_of(a, h);
            if (!differ) drop = reads_equal(x.b1, x.L1, y.b1, y.L1, false, lane) && (!PAIRS || reads_equal(x.b2, x.L2, y.b2, y.L2, false, lane));
            if (STRAND && !drop && try_flip) {
                flipped = PAIRS ? reads_equal(x.b1, x.L1, y.b2, y.L2, false, lane) && reads_equal(x.b2, x.L2, y.b1, y.L1, false, lane)
                                : reads_equal(x.b1, x.L1, y.b1, y.L1, true, lane);
                drop = flipped;
            }
        }
        if (lane == 0u) {
            const bool collision = h != r && !drop;
            kept += drop ? 0u : 1u;
            dropped += drop ? 1u : 0u;
            collisions += collision ? 1u : 0u;
            u64* const row = a.rows + r * KMX_DD_WORDS;
            unsigned long long count = 1u;
            if (collision) row[KMX_DD_COUNT] = 1u;   // (nobody adds to the COUNT of an item that is no head)
            else count = atomicAdd(reinterpret_cast<unsigned long long*>(a.rows + h * KMX_DD_WORDS + KMX_DD_COUNT), 1ull) + 1u;
            largest = count > largest ? count : largest;
            row[KMX_DD_REP] = drop ? h : r;
            row[KMX_DD_FLAGS] = (drop ? 0u : KMX_DD_F_KEPT) | (flipped ? KMX_DD_F_FLIPPED : 0u) | (collision ? KMX_DD_F_COLLISION : 0u) |
                                ((o_r & DD_OTHER) ? KMX_DD_F_OTHER : 0u);
            row[KMX_DD_HASH] = hc;
            if (a.keep) a.keep[r] = drop ? 0u : 1u;
        }
    }
    // (no atomics on the four words: a grid's worth of waves adding to one address costs more than the rest of the kernel)
    if (lane == 0u) {
        u64* const p = wave_partial + ((u64)blockIdx.x * WPR_WAVES + wv) * KMX_DD_SUMMARY_WORDS;
        p[KMX_DD_S_KEPT] = kept;
        p[KMX_DD_S_DROPPED] = dropped;
        p[KMX_DD_S_LARGEST] = largest;
        p[KMX_DD_S_COLLISIONS] = collisions;
    }
}

// the waves' partial summaries -> the summary: sums, and the maximum for the largest COUNT.  One block.
__global__ void __launch_bounds__(CT) reads_dedup_summary_kernel(const u64* __restrict__ wave_partial, u64 n_waves, unsigned long long* __restrict__ summary) {
    __shared__ u64 sh[CT / 64];
    u64 v[KMX_DD_SUMMARY_WORDS] = {0u, 0u, 0u, 0u};
    for (u64 w = threadIdx.x; w < n_waves; w += CT) {
#pragma unroll
        for (u32 q = 0; q < KMX_DD_SUMMARY_WORDS; ++q) {
            const u64 x = wave_partial[w * KMX_DD_SUMMARY_WORDS + q];
            v[q] = q == KMX_DD_S_LARGEST ? (x > v[q] ? x : v[q]) : v[q] + x;
        }
    }
#pragma unroll
    for (u32 q = 0; q < KMX_DD_SUMMARY_WORDS; ++q) {
        u64 t;
        if (q == KMX_DD_S_LARGEST) {
            u64 m = v[q];
            for (u32 o = 32; o > 0; o >>= 1) {
                const u64 x = __shfl_xor(m, o);
                m = x > m ? x : m;
            }
            if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = m;
            __syncthreads();
            t = 0;
            if (threadIdx.x == 0)
                for (u32 w = 0; w < CT / 64u; ++w) t = sh[w] > t ? sh[w] : t;
            __syncthreads();
        } else {
            t = block_sum(v[q], sh);
        }
        if (threadIdx.x == 0) summary[q] = t;
    }
}

// The work area: the records and their flag bytes (the sort's input), the counter's area, the sorted records, the counts the sort's
// emit writes (8 B per item: nobody reads them, and the group of every position and the head of every group, 4 B each, take their
// place once it is through), the items' bytes, the blocks' head counts, the partial summaries of the verify kernel's waves and the
// summary.
struct DedupArea {
    u64* rec;
    uint8_t* valid;
    void* count;
    u64* sorted;
    u64* counts;
    u32 *group, *head_item;
    uint8_t* other;
    u64* partial;
    u64* wave_partial;
    unsigned long long* summary;
};
size_t dedup_layout(u64 n, int n_cu, DedupArea* out, void* base) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += align256(bytes);
        return base ? static_cast<char*>(base) + at : nullptr;
    };
    DedupArea d{};
    d.rec = reinterpret_cast<u64*>(take(16u * n));
    d.valid = reinterpret_cast<uint8_t*>(take(n));
    d.count = take(count_area_bytes(2u, n));
    d.sorted = reinterpret_cast<u64*>(take(16u * n));
    d.counts = reinterpret_cast<u64*>(take(8u * n));
    d.group = reinterpret_cast<u32*>(d.counts);
    d.head_item = d.group + n;
    d.other = reinterpret_cast<uint8_t*>(take(n));
    d.partial = reinterpret_cast<u64*>(take(8u * (ceil_div(n, MCHUNK) + 2u)));
    d.wave_partial = reinterpret_cast<u64*>(take(8u * KMX_DD_SUMMARY_WORDS * WPR_WAVES * (size_t)wave_per_read_grid(n, n_cu)));
    d.summary = reinterpret_cast<unsigned long long*>(take(8u * KMX_DD_SUMMARY_WORDS));
    if (out) *out = d;
    return off;
}

}  // namespace

size_t reads_dedup_bytes(u64 n_reads, int n_cu) { return dedup_layout(n_reads, n_cu, nullptr, nullptr); }

hipError_t launch_reads_dedup(const ReadsDedup& a, void* area, unsigned long long* h_pinned, u64* h_summary, bool* bad, int n_cu, hipStream_t st) {
    const u64 n = a.n_reads;
    DedupArea d;
    dedup_layout(n, n_cu, &d, area);
    *bad = false;
    hipError_t e;
    const dim3 waves(wave_per_read_grid(n, n_cu));
    hipLaunchKernelGGL(reads_dedup_key_kernel, waves, dim3(WPR_THREADS), 0, st, a, d.rec, d.valid, d.other);
    u64 n_valid = 0, n_distinct = 0;
    if ((e = launch_count_sort(2u, d.rec, d.valid, n, 64u, d.count, h_pinned, &n_valid, &n_distinct, bad, st)) != hipSuccess) return e;
    if (*bad) return hipSuccess;
    if (n_valid != n || n_distinct != n) {   // (every record holds its item's index: all are distinct)
        *bad = true;
        return hipSuccess;
    }
    if ((e = launch_count_emit(2u, d.rec, n, n_valid, d.count, d.sorted, d.counts, st)) != hipSuccess) return e;
    const u64 nb = ceil_div(n, MCHUNK);
    hipLaunchKernelGGL(reads_dedup_head_count_kernel, dim3((unsigned)nb), dim3(CT), 0, st, (const u64*)d.sorted, n, d.partial);
    hipLaunchKernelGGL(scan_single_kernel, dim3(1), dim3(CT), 0, st, d.partial, nb, d.partial + nb);
    hipLaunchKernelGGL(reads_dedup_head_write_kernel, dim3((unsigned)nb), dim3(CT), 0, st, (const u64*)d.sorted, n, (const u64*)d.partial, d.group,
                       d.head_item);
    auto verify = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, waves, dim3(WPR_THREADS), 0, st, a, (const u64*)d.sorted, (const u32*)d.group, (const u32*)d.head_item,
                           (const uint8_t*)d.other, d.wave_partial);
    };
    if (a.pairs) {
        if (a.strand) verify(reads_dedup_verify_kernel<true, true>);
        else verify(reads_dedup_verify_kernel<true, false>);
    } else {
        if (a.strand) verify(reads_dedup_verify_kernel<false, true>);
        else verify(reads_dedup_verify_kernel<false, false>);
    }
    hipLaunchKernelGGL(reads_dedup_summary_kernel, dim3(1), dim3(CT), 0, st, (const u64*)d.wave_partial, (u64)waves.x * WPR_WAVES, d.summary);
    return read_back(h_pinned, d.summary, KMX_DD_SUMMARY_WORDS, h_summary, st);
}

}  // namespace kmx
