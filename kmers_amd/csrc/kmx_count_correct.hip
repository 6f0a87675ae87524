// kmx_count_correct.hip -- conservative two-sided spectral correction of substitution errors (kmx_count_correct_reads(2)): which
// bases of a read to replace, decided from what kmx_count_lookup_reads(2) leaves -- one u64 count and one flag byte per window -- and
// from searches of the table for the windows spelled with another base.  The rule is in include/kmx.h, in full; in short: a base no
// solid window covers, but at least min_cover valid ones do, is a CANDIDATE; a base `a` FIXES it when every valid window that covers
// it is solid with `a` in its place; exactly one fixing base is written, two or three are AMBIGUOUS and nothing is written.  Every
// decision is taken against the ORIGINAL bytes: the host copies the reads to the output first and this kernel stores only the
// corrected bytes there, so no lane ever reads what another one wrote.
//
// One wave per read, steps of 64 base positions, lane = position p.  A step loads the count and the flag of window p and takes two
// ballots, valid and solid; with the previous step's two ballots that is 128 bits of history, and since the windows that cover p are
// p - k + 1 .. p with k - 1 <= 63, a mask and a popcount over them answer "how many valid windows cover p" and "does a solid one".
// Windows before the read's first (the previous ballots start as 0) and behind its last (they load as invalid) drop out by
// themselves.
//   phase 1  every candidate lane spells ONE valid window that covers it (the last one), puts each of the three other bases at p, and
//            searches the three canonical words in lockstep.  A base that fails there cannot fix p: a necessary condition only, it
//            changes no answer, and it keeps a read that is weak throughout at three searches per base instead of 3 k.
//   phase 2  for every (position, base) that survived, the wave turns to it together: lane j spells the j-th window that covers
//            the position (at most k <= 64 of them) with the base in place, searches it, and one ballot says whether any valid window
//            came out below solid_min.
// The search is the lookup's (table_search, kmx_count_dir.h): the directory's bin when there is a directory, binary steps down to LINE
// keys, the line loaded at once, every directory entry clamped to n -- a table that is not sorted gives wrong answers, never an access
// outside the arrays.  Windows are spelled from the read's bytes (8 per load where 8 are left in the window): every byte read lies
// inside a valid window of the read.  Vector loads and stores only; no LDS, no atomics, no scratch.  The four words of a read's row
// are written by its wave in one store; every row and every corrected byte has exactly one writer, so repeated calls are
// bit-identical.  Reads of any length go through the same stepping loop: long reads are exact, not fast.
#include "kmx_count_dir.h"

namespace kmx {

namespace {

constexpr u32 CR_BLOCKS_PER_CU = 16;   // the grid's cap: a wave takes the reads of its index modulo the grid's waves

// bits [0, n) of a 64-bit mask, n <= 64
__device__ __forceinline__ u64 low_bits(u32 n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }

// the code of a byte that is one of ACGTacgt (encode_base without its check): A0 C1 G2 T3
__device__ __forceinline__ u32 base_code(u32 c) {
    const u32 i = (c >> 1) & 3u;
    return i ^ (i >> 1);
}

template <u32 W>
__device__ __forceinline__ void put_base(u64& lo, u64& hi, u32 i, u32 c) {
    if (W == 1u || i < 32u) lo |= (u64)c << (2u * (i & 31u));
    else hi |= (u64)c << (2u * (i - 32u));
}

// the forward word of the window s[0, k), all of its bytes valid: base i at bits [2i, 2i + 1] (the iterator's fw word)
template <u32 W>
__device__ __forceinline__ Key<W> spell(const uint8_t* __restrict__ s, u32 k) {
    u64 lo = 0, hi = 0;
    u32 i = 0;
    for (; i + 8u <= k; i += 8u) {
        u64 v;
        __builtin_memcpy(&v, s + i, 8);
        u32 g = 0;
#pragma unroll
        for (u32 j = 0; j < 8u; ++j) g |= base_code((u32)(v >> (8u * j)) & 0xFFu) << (2u * j);
        // (i is a multiple of 8: the 16 bits lie in one word)
        if (W == 1u || i < 32u) lo |= (u64)g << (2u * (i & 31u));
        else hi |= (u64)g << (2u * (i - 32u));
    }
    for (; i < k; ++i) put_base<W>(lo, hi, i, base_code(s[i]));
    if constexpr (W == 1u) return Key<1>{lo};
    else return Key<2>{lo, hi};
}

// x with the base at position i replaced by code c
template <u32 W>
__device__ __forceinline__ Key<W> with_base(Key<W> x, u32 i, u32 c) {
    if (W == 1u || i < 32u) x.lo = (x.lo & ~(3ull << (2u * (i & 31u)))) | ((u64)c << (2u * (i & 31u)));
    else if constexpr (W == 2u) x.hi = (x.hi & ~(3ull << (2u * (i - 32u)))) | ((u64)c << (2u * (i - 32u)));
    return x;
}

// min(x, rc(x)): the key a table holds for the word x
template <u32 W>
__device__ __forceinline__ Key<W> canonical_of(const Key<W>& x, u32 k) {
    const Key<W> r = x.revcomp(k);
    return r.less(x) ? r : x;
}

// A wave-uniform value moved into vector registers.  What the searches take -- the table's arrays, n, solid_min -- is only ever combined
// with per-lane values; left in scalar registers it competes there with the lane predicates of the lockstep searches (a pair each)
// and with the wave's loop state, and the compiler starts spilling scalar registers.  The vector file has the room.
template <typename T>
__device__ __forceinline__ T in_vgpr(T x) {
    static_assert(sizeof(T) == 8u, "a register pair");
    u64 v;
    __builtin_memcpy(&v, &x, 8);
    asm volatile("" : "+v"(v));
    __builtin_memcpy(&x, &v, 8);
    return x;
}

// the count kmx_count_lookup answers for a search's hit
__device__ __forceinline__ u64 count_at(const u64* __restrict__ tcounts, u64 hit) {
    if (hit == ~0ull) return 0u;
    return tcounts != nullptr ? tcounts[hit] : 1u;
}

// offsets == nullptr: uniform reads of L >= k bases, read r at bases + r * L, its windows at r * (L - k + 1); otherwise read r at
// bases + offsets[r] with the windows wo[r] .. wo[r + 1) (a read without a window: a row of zeros).  wcounts / wflags: one u64 and
// one byte per window, as the lookup leaves them.  `out` holds a copy of the reads and does not overlap them.
template <u32 W, bool DIR>
__global__ void __launch_bounds__(CT) correct_kernel(const uint8_t* __restrict__ bases_, uint8_t* __restrict__ out_, const u64* __restrict__ offsets,
                                                     const u64* __restrict__ wo, u64 n_reads, u32 L, const u64* __restrict__ wcounts_,
                                                     const uint8_t* __restrict__ wflags_, const u64* __restrict__ keys_,
                                                     const u64* __restrict__ tcounts_, u64 n_, u32 k, u32 p, const u32* __restrict__ dir_,
                                                     u64 solid_min_, u32 min_cover, u64* __restrict__ fixes) {
    using K = Key<W>;
    const u64* __restrict__ keys = in_vgpr(keys_);
    const u64* __restrict__ tcounts = in_vgpr(tcounts_);
    const u32* __restrict__ dir = in_vgpr(dir_);
    const u64 n = in_vgpr(n_), solid_min = in_vgpr(solid_min_);
    const u64* __restrict__ wcounts = in_vgpr(wcounts_);
    const uint8_t* __restrict__ wflags = in_vgpr(wflags_);
    const uint8_t* __restrict__ bases = in_vgpr(bases_);
    uint8_t* __restrict__ out = in_vgpr(out_);
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 stride = (u64)gridDim.x * (CT / 64u);
    // the windows that cover the position in this lane, as bits of this step's ballots and of the previous step's
    const u64 m_cur = low_bits(lane + 1u) & ~low_bits(lane + 1u >= k ? lane + 1u - k : 0u);
    const u64 m_prev = lane + 1u < k ? ~low_bits(65u + lane - k) : 0u;
    for (u64 r = (u64)blockIdx.x * (CT / 64u) + wave; r < n_reads; r += stride) {
        u64 b0, w0;
        u32 nwin;
        if (offsets != nullptr) {
            b0 = offsets[r];
            w0 = wo[r];
            nwin = (u32)(wo[r + 1u] - w0);   // (below 2^31: a longer read has no window)
        } else {
            b0 = r * L;
            nwin = L - k + 1u;
            w0 = r * nwin;
        }
        u32 n_weak = 0, n_cand = 0, n_corr = 0, n_amb = 0;   // per lane: summed over the wave behind the read's last step
        const uint8_t* __restrict__ rb = bases + b0;
        const u32 len = nwin != 0u ? nwin + k - 1u : 0u;
        u64 pv = 0, ps = 0;   // the previous step's ballots
        for (u32 s = 0; s < len; s += 64u) {
            const u32 pos = s + lane;
            bool v = false, sd = false;
            if (pos < nwin) {
                v = (wflags[w0 + pos] & KMX_WIN_VALID) != 0u;
                sd = v && wcounts[w0 + pos] >= solid_min;
            }
            const u64 cv = __ballot(v), cs = __ballot(sd);
            n_weak += v && !sd ? 1u : 0u;
            const u32 covered = (u32)__popcll(cv & m_cur) + (u32)__popcll(pv & m_prev);
            const bool any_solid = ((cs & m_cur) | (ps & m_prev)) != 0u;
            u32 c0 = 0;
            bool cand = false;
            if (pos < len) {
                c0 = rb[pos];
                cand = encode_base(c0) < 4u && covered >= min_cover && !any_solid;
            }
            const u32 code0 = base_code(c0);
            // phase 1: the three other bases on the last valid window that covers the position
            u32 surv = 0;
            if (cand && n != 0u) {
                const u64 a = cv & m_cur;
                const u32 wsel = a != 0u ? s + 63u - (u32)__clzll((long long)a) : s - 1u - (u32)__clzll((long long)(pv & m_prev));
                const K fw = spell<W>(rb + wsel, k);
                K q[3];
                const bool live[3] = {true, true, true};
                u64 hit[3];
#pragma unroll
                for (u32 j = 0; j < 3u; ++j) q[j] = canonical_of<W>(with_base<W>(fw, pos - wsel, (code0 + 1u + j) & 3u), k);
                table_search<W, DIR, 3>(keys, n, k, p, dir, q, live, hit);
#pragma unroll
                for (u32 j = 0; j < 3u; ++j)
                    if (count_at(tcounts, hit[j]) >= solid_min) surv |= 1u << j;
            }
            // phase 2: every window that covers a surviving position, a lane each
            u32 n_fix = 0, fix_code = 0;
            unsigned long long todo = __ballot(surv != 0u);
            while (todo) {
                const u32 src = (u32)__ffsll(todo) - 1u;
                todo &= todo - 1ull;
                const u32 sp = s + src;
                const u32 s_surv = (u32)__shfl((int)surv, (int)src), s_code0 = (u32)__shfl((int)code0, (int)src);
                const u32 w_lo = sp + 1u >= k ? sp + 1u - k : 0u, w_hi = sp < nwin ? sp : nwin - 1u;
                const u32 wj = w_lo + lane;
                const bool vj = wj <= w_hi && (wflags[w0 + wj] & KMX_WIN_VALID) != 0u;
                K fwj = K::sentinel();
                if (vj) fwj = spell<W>(rb + wj, k);
                u32 cnt = 0, code = 0;
#pragma unroll 1
                for (u32 j = 0; j < 3u; ++j) {
                    if (((s_surv >> j) & 1u) == 0u) continue;
                    const u32 alt = (s_code0 + 1u + j) & 3u;
                    bool below = false;
                    if (vj) {
                        const K q[1] = {canonical_of<W>(with_base<W>(fwj, sp - wj, alt), k)};
                        const bool live[1] = {true};
                        u64 hit[1];
                        table_search<W, DIR, 1>(keys, n, k, p, dir, q, live, hit);
                        below = count_at(tcounts, hit[0]) < solid_min;
                    }
                    if (__ballot(below) == 0ull) {
                        cnt += 1u;
                        code = alt;
                    }
                }
                if (lane == src) {
                    n_fix = cnt;
                    fix_code = code;
                }
            }
            const bool corr = cand && n_fix == 1u, amb = cand && n_fix >= 2u;
            if (corr) out[b0 + pos] = (uint8_t)(((0x54474341u >> (8u * fix_code)) & 0xFFu) | (c0 & 0x20u));   // 'A' 'C' 'G' 'T', in the byte's case
            n_cand += cand ? 1u : 0u;
            n_corr += corr ? 1u : 0u;
            n_amb += amb ? 1u : 0u;
            pv = cv;
            ps = cs;
        }
        if (fixes != nullptr) {
            // (a lane counts at most one per step and a read has fewer than 2^25 steps: the four counts ride in one u64 sum each pair)
            const u64 s01 = wave_sum(((u64)n_cand << 32) | n_weak), s23 = wave_sum(((u64)n_amb << 32) | n_corr);
            const u64 pair = lane < 2u ? s01 : s23;
            if (lane < KMX_CR_WORDS) fixes[KMX_CR_WORDS * r + lane] = (lane & 1u) ? pair >> 32 : pair & 0xFFFFFFFFull;
        }
    }
}

}  // namespace

// ---------------------------------------------------------------- host side
// dir_area: the directory launch_count_lookup built for this table (prefix bits p), or nullptr = the plain search
hipError_t launch_count_correct(u32 words, const uint8_t* bases, uint8_t* out, const u64* offsets, const u64* win_offsets, u64 n_reads, u32 L,
                                const u64* wcounts, const uint8_t* wflags, const u64* keys, const u64* tcounts, u64 n, u32 k, const void* dir_area,
                                u32 p, u64 solid_min, u32 min_cover, u64* fixes, int n_cu, hipStream_t st) {
    const u32* dir = static_cast<const u32*>(dir_area);
    u64 nb = ceil_div(n_reads, CT / 64u);
    const u64 cap = (u64)(n_cu > 0 ? n_cu : 256) * CR_BLOCKS_PER_CU;
    if (nb > cap) nb = cap;
    const dim3 grid((unsigned)(nb ? nb : 1u)), block(CT);
    with_width(words, [&](auto w) {
        constexpr u32 W = decltype(w)::value;
        if (dir) hipLaunchKernelGGL((correct_kernel<W, true>), grid, block, 0, st, bases, out, offsets, win_offsets, n_reads, L, wcounts, wflags, keys,
                                    tcounts, n, k, p, dir, solid_min, min_cover, fixes);
        else hipLaunchKernelGGL((correct_kernel<W, false>), grid, block, 0, st, bases, out, offsets, win_offsets, n_reads, L, wcounts, wflags, keys,
                                tcounts, n, k, p, dir, solid_min, min_cover, fixes);
    });
    return hipGetLastError();
}

}  // namespace kmx
