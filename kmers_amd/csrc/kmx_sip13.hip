// kmx_sip13.hip -- the minimizer calls under std's hashers: SipHash-1-3(key0, key1; the l-mer's 8 little-endian bytes), the
// hash_one(&DefaultHasher / RandomState, l-mer) of Kmer::minimizer_word (kmer.rs:170-192) and SeqVecMinimizerIter
// (seq_vector/minimizers.rs:39-141, hashes at :88,113).  include/kmx.h: kmx_minimizer_words_sip13, kmx_seqvec_minimizers_sip13,
// kmx_minimizers_sip13.
//
// The sliding-minimum kernels of the Lex / identity calls (kmx_minimizers.hip, kmx_seqvec.hip) pack (hash << 8) | position into
// one u64 key, which leaves 56 bits for the hash; SipHash has 64.  Here the hash and the position stay apart:
//   * a WAVE owns a piece of at most 256 bases of one read (a longer read is walked piece by piece: pieces of T = 257 - k k-mers
//     that overlap by k - 1 bases, as the Lex kernel cuts uniform reads);
//   * the piece is packed to 2-bit codes in the wave's LDS slice (16 bases per dword), every l-mer is hashed ONCE into a u64
//     array beside it (hash_of[p], p = its position in the piece);
//   * k-mer i takes the minimum of hash_of[i .. i + k - w] with a strict `<` in increasing position: the leftmost of equal hashes,
//     the tie rule of the reference's monotone deque (minimizers.rs:61-81, `backmer.hash <= dqmer.hash` keeps the earlier one);
//   * the l-mer itself comes back out of the packed piece at the winning position.
// No block barrier: the waves of a block work on unrelated pieces.  k above 256 bases: minimizers_sip_generic_kernel.  The call is bound by VALU issue (five SipRounds per l-mer,
// then k - w compares per k-mer), not by HBM.
#include "kmx_device.h"
#include "kmx_launch.h"

namespace kmx {

constexpr u32 SIP_PIECE = 256u;                  // bases of a piece
constexpr u32 SIP_PK_DWORDS = SIP_PIECE / 16u + 2u;   // packed piece + 2 dwords the field reads look ahead into

// the 2w-bit field at base p of a packed piece (w in [1, 32]); reads dwords q, q + 1, q + 2
__device__ __forceinline__ u64 sip_field(const u32* __restrict__ pk, u32 p, u32 w) {
    const u32 q = p >> 4, sh = 2u * (p & 15u);
    const u64 lo = (u64)pk[q] | ((u64)pk[q + 1u] << 32);
    const u64 v = sh ? ((lo >> sh) | ((u64)pk[q + 2u] << (64u - sh))) : lo;
    return v & mask2k(w);
}

__device__ __forceinline__ void sip_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Kmer::minimizer_word(word, k, width, &state) with a SipHash state: a lane per word, the running minimum starts at u64::MAX and
// only a strictly smaller hash replaces it (kmer.rs:176-189)
__global__ void __launch_bounds__(256)
minimizer_words_sip_kernel(const u64* __restrict__ in, u64 n, u32 k, u32 w, SipKey key, u64* __restrict__ out_mm, u32* __restrict__ out_off) {
    const u64 mask = mask2k(w);
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const u64 word = in[e];
        u64 best = word & mask, best_h = ~0ull;
        u32 off = 0;
        for (u32 pos = 0; pos + w <= k; ++pos) {
            const u64 mm = (word >> (2u * pos)) & mask;   // sub_kmer_word, kmer.rs:156-162
            const u64 h = siphash13(mm, key);
            if (h < best_h) {
                best = mm;
                best_h = h;
                off = pos;
            }
        }
        out_mm[e] = best;
        out_off[e] = off;
    }
}

// where the reads lie.  ASCII: read r = bases[offsets[r], offsets[r+1]) or bases[r L, (r+1) L); PACKED: read r = the slice
// [r L, (r+1) L) of a SeqVector (n_bases = n_reads L bases in `words`, base i at flat bits [2i, 2i+1]).
struct SipReads {
    const uint8_t* bases;
    const u64* words;
    const u64* offsets;
    const u64* win_offsets;
    u64 n_reads;
    u32 L;
};

template <bool PACKED>
__global__ void __launch_bounds__(256)
minimizers_sip_kernel(const SipReads rd, u32 k, u32 w, SipKey key, u64* __restrict__ out_word, u32* __restrict__ out_pos,
                      unsigned long long* __restrict__ first_bad) {
    __shared__ u32 pk_all[4][SIP_PK_DWORDS];
    __shared__ u64 hash_all[4][SIP_PIECE];
    const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    u32* const pk = pk_all[wv];
    u64* const hash_of = hash_all[wv];
    const u32 T = SIP_PIECE + 1u - k, span = k - w + 1u;   // (k <= SIP_PIECE: the launchers send larger k to the generic kernel)
    if (k > SIP_PIECE) return;
    const u64 wave = (u64)blockIdx.x * 4u + wv, n_waves = (u64)gridDim.x * 4u;
    const u64 n_bases = rd.n_reads * (u64)rd.L;   // (PACKED)
    for (u64 r = wave; r < rd.n_reads; r += n_waves) {
        u64 o0 = r * (u64)rd.L, len = rd.L, slot0 = r * (u64)(rd.L >= k ? rd.L - k + 1u : 0u);
        if (!PACKED && rd.offsets) {
            o0 = rd.offsets[r];
            len = rd.offsets[r + 1u] - o0;
            slot0 = rd.win_offsets[r];
        }
        bool bad = false;
        for (u64 pb = 0;; pb += T) {
            const u32 plen = (u32)(len - pb < (u64)(T + k - 1u) ? len - pb : (u64)(T + k - 1u));   // bases of this piece
            // ---- the piece, packed: dword d = its bases [16 d, 16 d + 16); codes past plen are 0
            if constexpr (PACKED) {
                for (u32 d = lane; d < SIP_PK_DWORDS; d += 64u) {
                    const u64 pos = o0 + pb + 16u * d;
                    u32 v = 0;
                    if (16u * d < plen) {
                        const u64 wi = pos >> 5;
                        const u32 sh = 2u * (u32)(pos & 31u);
                        const u64 lo = rd.words[wi];
                        const u64 hi = (sh > 32u && wi + 1u < (n_bases + 31u) / 32u) ? rd.words[wi + 1u] : 0ull;
                        v = (u32)(sh ? ((lo >> sh) | (hi << (64u - sh))) : lo);
                        const u32 in = plen - 16u * d;
                        if (in < 16u) v &= (1u << (2u * in)) - 1u;
                    }
                    pk[d] = v;
                }
            } else {
                // four bases per lane (byte loads: the piece may start at any address), 8 bits of codes per lane
                const uint8_t* const s = rd.bases + o0 + pb;
                u32 codes = 0;
#pragma unroll
                for (u32 j = 0; j < 4u; ++j) {
                    const u32 p = 4u * lane + j;
                    if (p < plen) {
                        const u32 c = s[p];
                        bad |= encode_base(c) >= 4u;
                        const u32 i = (c >> 1) & 3u;        // what SeqVector::from would pack (kmx.h: a bad byte spells (c >> 1) & 3)
                        codes |= (i ^ (i >> 1)) << (2u * j);
                    }
                }
                reinterpret_cast<uint8_t*>(pk)[lane] = (uint8_t)codes;
                if (lane < SIP_PK_DWORDS - SIP_PIECE / 16u) pk[SIP_PIECE / 16u + lane] = 0u;
            }
            sip_wave_sync();
            // ---- every l-mer of the piece hashed once
            const u32 nl = plen >= w ? plen - w + 1u : 0u;
            for (u32 p = lane; p < nl; p += 64u) hash_of[p] = siphash13(sip_field(pk, p, w), key);
            sip_wave_sync();
            // ---- k-mer i: the leftmost minimum of hash_of[i, i + span)
            const u32 nk = plen >= k ? plen - k + 1u : 0u;
            for (u32 i = lane; i < nk; i += 64u) {
                u64 bh = hash_of[i];
                u32 best = i;
                for (u32 q = 1; q < span; ++q) {
                    const u64 h = hash_of[i + q];
                    if (h < bh) {
                        bh = h;
                        best = i + q;
                    }
                }
                const u64 slot = slot0 + pb + i;
                __builtin_nontemporal_store(sip_field(pk, best, w), &out_word[slot]);
                __builtin_nontemporal_store((u32)(pb + best), &out_pos[slot]);
            }
            sip_wave_sync();   // (the next piece overwrites the arrays)
            if (pb + T + k - 1u >= len) break;
        }
        if (!PACKED && __any(bad) && lane == 0u) atomicMin(first_bad, (unsigned long long)r);
    }
}

// k above a piece (k > 256): a wave per read, a lane per k-mer, the window's k - w + 1 l-mers rolled base by base from the read and
// hashed one after the other (strict `<`: the leftmost of equal hashes).  Each l-mer is hashed once per window that holds it -- this
// is the fallback for what the piece kernel cannot hold, not a fast path.
template <bool PACKED>
__global__ void __launch_bounds__(256)
minimizers_sip_generic_kernel(const SipReads rd, u32 k, u32 w, SipKey key, u64* __restrict__ out_word, u32* __restrict__ out_pos,
                              unsigned long long* __restrict__ first_bad) {
    const u32 lane = threadIdx.x & 63u;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((u64)gridDim.x * blockDim.x) >> 6;
    const u32 span = k - w + 1u, top = 2u * (w - 1u);
    for (u64 r = wave; r < rd.n_reads; r += n_waves) {
        u64 o0 = r * (u64)rd.L, len = rd.L, slot0 = r * (u64)(rd.L >= k ? rd.L - k + 1u : 0u);
        if (!PACKED && rd.offsets) {
            o0 = rd.offsets[r];
            len = rd.offsets[r + 1u] - o0;
            slot0 = rd.win_offsets[r];
        }
        auto code = [&](u64 at) -> u64 {
            if constexpr (PACKED) {
                const u64 pos = o0 + at;
                return (rd.words[pos >> 5] >> (2u * (u32)(pos & 31u))) & 3ull;
            } else {
                const u32 i = (rd.bases[o0 + at] >> 1) & 3u;
                return (u64)(i ^ (i >> 1));
            }
        };
        if constexpr (!PACKED) {
            bool bad = false;
            for (u64 i = lane; i < len; i += 64u) bad |= encode_base(rd.bases[o0 + i]) >= 4u;
            if (__any(bad) && lane == 0u) atomicMin(first_bad, (unsigned long long)r);
        }
        for (u64 i = lane; i + k <= len; i += 64u) {
            u64 lm = 0;
            for (u32 b = 0; b < w; ++b) lm |= code(i + b) << (2u * b);
            u64 best = lm, bh = siphash13(lm, key);
            u32 bp = 0;
            for (u32 q = 1; q < span; ++q) {
                lm = (lm >> 2) | (code(i + q + w - 1u) << top);
                const u64 h = siphash13(lm, key);
                if (h < bh) {
                    bh = h;
                    best = lm;
                    bp = q;
                }
            }
            out_word[slot0 + i] = best;
            out_pos[slot0 + i] = (u32)(i + bp);
        }
    }
}

static inline unsigned sip_grid(u64 n_waves_wanted, int n_cu) {
    u64 g = (n_waves_wanted + 3u) / 4u;
    const u64 cap = (u64)n_cu * 16u;
    if (g > cap) g = cap;
    return (unsigned)(g ? g : 1);
}

hipError_t launch_minimizer_words_sip(const u64* in, u64 n, u32 k, u32 w, u64 k0, u64 k1, u64* out_mm, u32* out_off, int n_cu,
                                      hipStream_t st) {
    u64 g = (n + 255u) / 256u;
    const u64 cap = (u64)n_cu * 16u;
    if (g > cap) g = cap;
    hipLaunchKernelGGL(minimizer_words_sip_kernel, dim3((unsigned)(g ? g : 1)), dim3(256), 0, st, in, n, k, w, sip_key(k0, k1), out_mm, out_off);
    return hipGetLastError();
}

// reads in ASCII (offsets == nullptr: uniform reads of L bases); first_bad: the lowest read index with a byte outside ACGTacgt
hipError_t launch_minimizers_reads_sip(const uint8_t* bases, const u64* offsets, const u64* win_offsets, u64 n_reads, u32 L, u32 k, u32 w,
                                       u64 k0, u64 k1, u64* out_word, u32* out_pos, unsigned long long* first_bad, int n_cu, hipStream_t st) {
    const SipReads rd{bases, nullptr, offsets, win_offsets, n_reads, L};
    if (k > SIP_PIECE) {   // (no piece of 256 bases holds a k-mer)
        hipLaunchKernelGGL(minimizers_sip_generic_kernel<false>, dim3(sip_grid(n_reads, n_cu)), dim3(256), 0, st, rd, k, w, sip_key(k0, k1),
                           out_word, out_pos, first_bad);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(minimizers_sip_kernel<false>, dim3(sip_grid(n_reads, n_cu)), dim3(256), 0, st, rd, k, w, sip_key(k0, k1), out_word,
                       out_pos, first_bad);
    return hipGetLastError();
}

// read slices [r L, (r+1) L) of a SeqVector
hipError_t launch_seqvec_minimizers_sip(const u64* words, u64 n_reads, u32 L, u32 k, u32 w, u64 k0, u64 k1, u64* out_word, u32* out_pos,
                                        int n_cu, hipStream_t st) {
    const SipReads rd{nullptr, words, nullptr, nullptr, n_reads, L};
    if (k > SIP_PIECE) {
        hipLaunchKernelGGL(minimizers_sip_generic_kernel<true>, dim3(sip_grid(n_reads, n_cu)), dim3(256), 0, st, rd, k, w, sip_key(k0, k1),
                           out_word, out_pos, nullptr);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(minimizers_sip_kernel<true>, dim3(sip_grid(n_reads, n_cu)), dim3(256), 0, st, rd, k, w, sip_key(k0, k1), out_word,
                       out_pos, nullptr);
    return hipGetLastError();
}

}  // namespace kmx
