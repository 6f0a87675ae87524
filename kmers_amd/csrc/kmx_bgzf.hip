// kmx_bgzf.hip -- BGZF on the device: the block index of a compressed image, and its inflation, one wave per block.
//
// BUILD-DEFINED: the reference reads no files.  A BGZF file is a chain of gzip members of at most 64 KiB, each an independent DEFLATE
// stream: the one form of gzip with something to run in parallel over.
//   index:   one lane per byte marks the header patterns (candidates), compacted in ascending order (counts per KiB, a scan, the
//            write); each candidate's successor is found by a binary search for pos + BSIZE + 1; the candidates reachable from byte 0
//            are marked by pointer doubling over ping-pong jump arrays (in round r every marked j marks jump[j], then jump =
//            jump[jump]: after r rounds exactly the chain nodes at distance below 2^r are marked); the marked are ranked by a scan and
//            written, ISIZE beside them, and the ISIZE words scanned.
//   inflate: one wave per block, four waves a workgroup.  The serial core (kmx_bgzf_decode.h) runs wave-uniformly: every lane holds
//            the same bit buffer and decodes the same symbol from tables in LDS that all 64 lanes built.  Literals gather in a pending
//            64-byte tile (lane = position & 63) flushed by one store; stored blocks and matches are copied by all lanes.
//   crc:     a second kernel: each lane the plain CRC-32 of a contiguous piece, the pieces joined by multiplication with x^(8 len).
//   deflate: one wave per block of text, one wave a workgroup.  The parse goes in steps of 64 positions, a lane per
//            position; the codes are built by the serial core (kmx_bgzf_encode.h) run wave-uniformly; the bits go through a staging
//            window in LDS into a worst-case slot per block; the sizes are scanned and a copy kernel writes header, payload and
//            footer back to back.
#include "kmx_device.h"
#include "kmx_launch.h"
#include "kmx_bgzf_decode.h"
#include "kmx_bgzf_encode.h"

namespace kmx {

namespace {

constexpr u32 BZ_THREADS = 256;
constexpr u32 BZ_WAVES = BZ_THREADS / 64u;
constexpr u32 BZ_UNIT = 1024;              // bytes of the file a wave looks through per step of the candidate passes
constexpr u32 BZ_SCAN_THREADS = 1024, BZ_SCAN_ITEMS = 8;

__device__ __forceinline__ u32 lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ u32 lanes_below(u64 m) {
    return __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
}
__device__ __forceinline__ u32 uni(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ u64 uni64(u64 v) { return (u64)uni((u32)v) | ((u64)uni((u32)(v >> 32)) << 32); }
// the lanes of a wave have written LDS / memory that other lanes of it read next: the wave's memory operations are performed in
// order, the fence keeps the compiler from moving them across
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// a complete block may start at p: the header pattern, a size of at least 28, inside the file
__device__ __forceinline__ bool candidate_at(const uint8_t* __restrict__ f, u64 n, u64 p, u32* size) {
    if (p + bgzf::HEADER_BYTES > n || f[p] != 0x1f) return false;
    return bgzf::header_ok(f + p, size) && *size >= bgzf::MIN_BLOCK && p + *size <= n;
}

// ---- index, passes 1 and 3: candidates per unit of 1 KiB / their positions, ascending (WRITE: unit_counts holds the exclusive sums)
template <bool WRITE>
__global__ void __launch_bounds__(BZ_THREADS)
bgzf_candidates_kernel(const uint8_t* __restrict__ f, u64 n, u64 n_units, u32* __restrict__ unit_counts, u64* __restrict__ pos) {
    const u64 stride = (u64)gridDim.x * BZ_WAVES;
    for (u64 u = (u64)blockIdx.x * BZ_WAVES + (threadIdx.x >> 6); u < n_units; u += stride) {
        u32 running = WRITE ? unit_counts[u] : 0u;
        for (u32 it = 0; it < BZ_UNIT / 64u; ++it) {
            const u64 p = u * BZ_UNIT + it * 64u + lane_id();
            u32 size;
            const bool is = p < n && candidate_at(f, n, p, &size);
            const u64 m = __ballot(is);
            if (WRITE && is) pos[running + lanes_below(m)] = p;
            running += (u32)__builtin_popcountll(m);
        }
        if (!WRITE && lane_id() == 0u) unit_counts[u] = running;
    }
}

// ---- exclusive scan of a[0, n) in place by one block; *total = the sum.  (The arrays here have one word per KiB of file, per
// candidate or per block: a few 1e5 words for a file of gigabytes.)
template <class T>
__global__ void __launch_bounds__(BZ_SCAN_THREADS) bgzf_scan_kernel(T* __restrict__ a, u64 n, unsigned long long* __restrict__ total) {
    __shared__ u64 wave_sum[BZ_SCAN_THREADS / 64u];
    u64 carry = 0;
    for (u64 base = 0; base < n; base += (u64)BZ_SCAN_THREADS * BZ_SCAN_ITEMS) {
        const u64 i0 = base + (u64)threadIdx.x * BZ_SCAN_ITEMS;
        u64 v[BZ_SCAN_ITEMS];
        u64 sum = 0;
#pragma unroll
        for (u32 q = 0; q < BZ_SCAN_ITEMS; ++q) {
            v[q] = i0 + q < n ? (u64)a[i0 + q] : 0ull;
            sum += v[q];
        }
        u64 incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u64 o = __shfl_up(incl, d, 64);
            if (lane_id() >= (u32)d) incl += o;
        }
        __syncthreads();                 // wave_sum may still be read from the step before
        if (lane_id() == 63u) wave_sum[threadIdx.x >> 6] = incl;
        __syncthreads();
        u64 before = carry, all = 0;
#pragma unroll
        for (u32 w = 0; w < BZ_SCAN_THREADS / 64u; ++w) {
            const u64 x = wave_sum[w];
            before += w < (threadIdx.x >> 6) ? x : 0ull;
            all += x;
        }
        u64 run = before + incl - sum;
#pragma unroll
        for (u32 q = 0; q < BZ_SCAN_ITEMS; ++q) {
            if (i0 + q < n) a[i0 + q] = (T)run;
            run += v[q];
        }
        carry += all;
    }
    if (threadIdx.x == 0) *total = carry;
}

// ---- index, pass 4: the successor of every candidate (index C: none), and the first mark
__global__ void __launch_bounds__(BZ_THREADS)
bgzf_successor_kernel(const uint8_t* __restrict__ f, const u64* __restrict__ pos, u32 C, u32* __restrict__ jump, u32* __restrict__ mark) {
    const u32 stride = gridDim.x * BZ_THREADS;
    for (u32 j = blockIdx.x * BZ_THREADS + threadIdx.x; j <= C; j += stride) {
        if (j == C) {
            jump[j] = C;
            mark[j] = 0;
            continue;
        }
        const u64 p = pos[j];
        const u64 target = p + ((u32)f[p + 16u] | ((u32)f[p + 17u] << 8)) + 1u;
        u32 lo = j + 1u, hi = C;          // the first candidate at or behind target
        while (lo < hi) {
            const u32 mid = lo + (hi - lo) / 2u;
            if (pos[mid] < target) lo = mid + 1u; else hi = mid;
        }
        jump[j] = lo < C && pos[lo] == target ? lo : C;
        mark[j] = j == 0u && p == 0u ? 1u : 0u;
    }
}
// one round of the doubling: marked j marks jump[j]; next = jump[jump]
__global__ void __launch_bounds__(BZ_THREADS)
bgzf_mark_round_kernel(const u32* __restrict__ jump, u32* __restrict__ next, u32* mark, u32 C) {
    const u32 stride = gridDim.x * BZ_THREADS;
    for (u32 j = blockIdx.x * BZ_THREADS + threadIdx.x; j <= C; j += stride) {
        const u32 t = jump[j] <= C ? jump[j] : C;
        if (j < C && t < C && mark[j]) mark[t] = 1u;     // (a mark seen early marks a node of the chain all the same)
        next[j] = t < C ? (jump[t] <= C ? jump[t] : C) : C;
    }
}
// the marked: rank[] = the marks (to be scanned), stats[0] += ISIZE, stats[1] = max end, stats[5] = max start (the last block's)
__global__ void __launch_bounds__(BZ_THREADS)
bgzf_chain_stats_kernel(const uint8_t* __restrict__ f, const u64* __restrict__ pos, const u32* __restrict__ mark, u32 C, u32* __restrict__ rank,
                        unsigned long long* __restrict__ stats) {
    const u32 stride = gridDim.x * BZ_THREADS;
    for (u32 j = blockIdx.x * BZ_THREADS + threadIdx.x; j < C; j += stride) {
        const u32 mk = mark[j];
        rank[j] = mk;
        if (!mk) continue;
        const u64 p = pos[j];
        const u64 end = p + ((u32)f[p + 16u] | ((u32)f[p + 17u] << 8)) + 1u;
        atomicAdd(&stats[0], (unsigned long long)bgzf::le32(f + end - 4u));
        atomicMax(&stats[1], (unsigned long long)end);
        atomicMax(&stats[5], (unsigned long long)p);
    }
}
__global__ void __launch_bounds__(BZ_THREADS)
bgzf_write_index_kernel(const uint8_t* __restrict__ f, const u64* __restrict__ pos, const u32* __restrict__ mark, const u32* __restrict__ rank, u32 C,
                        u64 n_blocks, u64 end, u64* __restrict__ block_offsets, u64* __restrict__ text_offsets) {
    const u32 stride = gridDim.x * BZ_THREADS;
    for (u32 j = blockIdx.x * BZ_THREADS + threadIdx.x; j <= C; j += stride) {
        if (j == C) {
            block_offsets[n_blocks] = end;
            text_offsets[n_blocks] = 0;
            continue;
        }
        if (!mark[j]) continue;
        const u64 p = pos[j], b = rank[j];
        if (b >= n_blocks) continue;
        const u64 e = p + ((u32)f[p + 16u] | ((u32)f[p + 17u] << 8)) + 1u;
        block_offsets[b] = p;
        text_offsets[b] = bgzf::le32(f + e - 4u);
    }
}

// ---- inflate
// The code of one set built by the wave: counts per length and each symbol's rank within its length from one pass of ballots
// (symbols lane, lane + 64, ...), the first codes (serial, 15 steps), then every lane places its symbols.  NCH = chunks of 64 symbols.
template <u32 NCH>
__device__ __forceinline__ u32 build_code(const bgzf::Code& c, const uint8_t* lens, u32 n, u32 lane) {
    if (lane < 16u) c.count[lane] = 0;
    wave_sync();
    u32 rank[NCH], len[NCH];
#pragma unroll
    for (u32 ch = 0; ch < NCH; ++ch) {
        const u32 s = ch * 64u + lane;
        const u32 L = s < n ? (lens[s] & 15u) : 0u;
        u32 r = 0;
        for (u32 l = 1; l < 16u; ++l) {
            const u64 m = __ballot(L == l);
            if (m == 0ull) continue;
            const u32 cur = c.count[l];                       // (every lane reads and writes the same value: no lane depends on another's store)
            if (L == l) r = cur + lanes_below(m);
            c.count[l] = (uint16_t)(cur + (u32)__builtin_popcountll(m));
        }
        rank[ch] = r;
        len[ch] = L;
    }
    const u32 st = uni(bgzf::kraft_and_first(c, 1u));
    if (st) return st;
    bgzf::clear_table(c, lane, 64u);
    wave_sync();
#pragma unroll
    for (u32 ch = 0; ch < NCH; ++ch) bgzf::place_symbol(c, ch * 64u + lane, len[ch], rank[ch]);
    wave_sync();
    return 0;
}

// the pending tile: bytes [pend, produced) of the block's output sit in the lanes (lane = position & 63), all inside one tile
__device__ __forceinline__ void flush_tile(uint8_t* out, u32 pend, u32 produced, u32 tile, u32 lane) {
    const u32 at = (pend & ~63u) + lane;
    if (at >= pend && at < produced) out[at] = (uint8_t)tile;
}

// block b, by one wave.  Returns its status (uniform).
__device__ __forceinline__ u32 inflate_block(const uint8_t* __restrict__ file, u64 n_bytes, const u64* __restrict__ boff, const u64* __restrict__ toff, u64 b, u64 span,
                             uint8_t* text, bgzf::Work* w, u32 lane) {
    const u64 s = uni64(boff[b]), e = uni64(boff[b + 1u]);
    const u64 t0 = uni64(toff[0]), ta = uni64(toff[b]), tb = uni64(toff[b + 1u]);
    if (e > n_bytes || e < s || e - s < bgzf::MIN_BLOCK || e - s > 65536u) return KMX_BGZF_ST_HEADER;
    if (ta < t0 || tb < ta || tb - t0 > span || tb - ta > 0xFFFFFFFFull) return KMX_BGZF_ST_LENGTH;
    const u32 room = (u32)(tb - ta);
    const uint8_t* p = file + s;
    u32 size;
    if (!bgzf::header_ok(p, &size) || size != (u32)(e - s)) return KMX_BGZF_ST_HEADER;
    if (uni(bgzf::le32(p + size - 4u)) != room) return KMX_BGZF_ST_LENGTH;
    uint8_t* out = text + (ta - t0);
    bgzf::Bits bits = bgzf::open_bits(p + bgzf::HEADER_BYTES, size - bgzf::HEADER_BYTES - bgzf::FOOTER_BYTES);
    const bgzf::Code lit = bgzf::lit_code(w), dist = bgzf::dist_code(w);
    u32 produced = 0, pend = 0, tile = 0;
    for (;;) {
        u32 fin, kind;
        u32 st = uni(bgzf::block_header(bits, &fin, &kind));
        if (st) return st;
        fin = uni(fin);
        kind = uni(kind);
        if (kind == 0u) {
            u32 len = 0;
            st = uni(bgzf::stored_header(bits, &len));
            if (st) return st;
            len = uni(len);
            bits.pos = uni(bits.pos);
            if (len > room - produced) return KMX_BGZF_ST_STORED;
            flush_tile(out, pend, produced, tile, lane);
            for (u32 i = lane; i < len; i += 64u) out[produced + i] = bits.p[bits.pos + i];
            bgzf::skip_bytes(bits, len);
            produced += len;
            pend = produced;
        } else {
            u32 hlit, hdist;
            if (kind == 1u) {
                bgzf::fixed_lengths(w, lane, 64u, &hlit, &hdist);
            } else {
                st = uni(bgzf::dynamic_lengths(bits, w, &hlit, &hdist));
                if (st) return st;
                hlit = uni(hlit);
                hdist = uni(hdist);
                bits.pos = uni(bits.pos);
                bits.cnt = uni(bits.cnt);
                bits.buf = uni64(bits.buf);
            }
            wave_sync();
            st = build_code<5>(lit, w->lens, hlit, lane);
            if (st) return st;
            st = build_code<1>(dist, w->lens + (kind == 1u ? bgzf::MAX_LIT : hlit), hdist, lane);
            if (st) return st;
            for (;;) {
                bgzf::Token t = bgzf::next_token(bits, lit, dist, produced, room);
                t.kind = uni(t.kind);
                t.a = uni(t.a);
                bits.pos = uni(bits.pos);
                bits.cnt = uni(bits.cnt);
                bits.buf = uni64(bits.buf);
                if (t.kind == 0u) {
                    tile = lane == (produced & 63u) ? t.a : tile;
                    produced += 1u;
                    if ((produced & 63u) == 0u) {
                        flush_tile(out, pend, produced, tile, lane);
                        pend = produced;
                    }
                } else if (t.kind == 1u) {
                    const u32 len = t.a, D = uni(t.d);
                    flush_tile(out, pend, produced, tile, lane);
                    // Sources older than this match were stored by other lanes of this wave in earlier instructions.  A wave's vector
                    // memory operations are performed in order, so the loads below see them; the wavefront-scope fence is what keeps
                    // the compiler from reordering the two (it emits no instruction).
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    const uint8_t* src = out + (produced - D);
                    for (u32 i = lane; i < len; i += 64u) out[produced + i] = src[D >= len ? i : i % D];
                    produced += len;
                    pend = produced;
                } else if (t.kind == 2u) {
                    break;
                } else {
                    return t.a;
                }
            }
        }
        if (fin) break;
    }
    flush_tile(out, pend, produced, tile, lane);
    return produced == room ? 0u : (u32)KMX_BGZF_ST_LENGTH;
}

__global__ void __launch_bounds__(BZ_THREADS)
bgzf_inflate_kernel(const uint8_t* __restrict__ file, u64 n_bytes, const u64* __restrict__ boff, const u64* __restrict__ toff, u64 n_blocks, u64 span,
                    uint8_t* text, u32* __restrict__ status) {
    __shared__ bgzf::Work work[BZ_WAVES];
    const u32 wave = threadIdx.x >> 6;
    const u64 b = (u64)blockIdx.x * BZ_WAVES + wave;
    if (b >= n_blocks) return;
    const u32 st = inflate_block(file, n_bytes, boff, toff, b, span, text, &work[wave], lane_id());
    if (lane_id() == 0u) status[b] = st;
}

// The CRC-32 of out[0, room) by one wave (uniform): each lane the plain CRC of a contiguous piece over the table `tab` (256 words
// in LDS), the pieces joined by multiplication with x^(8 * bytes behind the piece).
__device__ __forceinline__ u32 wave_crc32(const u32* tab, const uint8_t* __restrict__ out, u32 room, u32 lane) {
    const u32 piece = (room + 63u) / 64u;
    const u32 lo = lane * piece < room ? lane * piece : room, hi = lo + piece < room ? lo + piece : room;
    u32 crc = 0;
    u32 i = lo;
    for (; i + 4u <= hi; i += 4u) {      // four bytes a load (any alignment), four table steps
        crc ^= bgzf::load32(out + i);
#pragma unroll
        for (int q = 0; q < 4; ++q) crc = tab[crc & 255u] ^ (crc >> 8);
    }
    for (; i < hi; ++i) crc = tab[(crc ^ out[i]) & 255u] ^ (crc >> 8);
    crc = bgzf::crc_mul(crc, bgzf::crc_x_pow_bytes(room - hi));
    for (int o = 32; o > 0; o >>= 1) crc ^= __shfl_xor(crc, o, 64);
    return bgzf::crc_finish(crc, room);
}

// the CRC-32 of every block that decoded, against its footer; the lowest bad block
__global__ void __launch_bounds__(BZ_THREADS)
bgzf_crc_kernel(const uint8_t* __restrict__ file, const u64* __restrict__ boff, const u64* __restrict__ toff, u64 n_blocks, const uint8_t* __restrict__ text,
                u32* __restrict__ status, unsigned long long* __restrict__ first_bad, u32 check) {
    __shared__ u32 tab[256];
    tab[threadIdx.x] = bgzf::crc_table_entry(threadIdx.x);
    __syncthreads();
    const u64 b = (u64)blockIdx.x * BZ_WAVES + (threadIdx.x >> 6);
    if (b >= n_blocks) return;
    const u32 lane = lane_id();
    u32 st = uni(status[b]);
    if (st == 0u && check) {
        // (status 0: the decode kernel has checked the offsets and the header of this block)
        const u64 t0 = uni64(toff[0]), ta = uni64(toff[b]);
        const u32 room = (u32)(uni64(toff[b + 1u]) - ta);
        const u32 want = bgzf::le32(file + uni64(boff[b + 1u]) - 8u);
        if (wave_crc32(tab, text + (ta - t0), room, lane) != want) {
            st = KMX_BGZF_ST_CRC;
            if (lane == 0u) status[b] = st;
        }
    }
    if (st != 0u && lane == 0u) atomicMin(first_bad, (unsigned long long)b);
}

// ---- deflate: one wave per BGZF block, one wave a workgroup; the serial core is kmx_bgzf_encode.h
constexpr u32 BZ_DEFLATE_THREADS = 64;
constexpr u32 BZ_STORED_BIT = 0x80000000u;       // pay[b]: the payload's bytes, and this bit for a stored block

// One code by the wave: every lane ranks its own symbols (symbols lane, lane + 64, ...) into w->order, then all lanes run the serial
// construction alike -- the same loads, the same stores of the same values -- so no lane waits for another's result.
template <u32 NCH>
__device__ __forceinline__ void enc_build(bgzf::EncWork* w, const u32* freq, u32 n, u32 limit, uint8_t* len, uint16_t* code, bool complete, u32 lane) {
    u32 m = 0;
#pragma unroll
    for (u32 ch = 0; ch < NCH; ++ch) {
        const u32 s = ch * 64u + lane;
        const u32 f = s < n ? freq[s] : 0u;
        if (f) w->order[bgzf::enc_rank(freq, n, s)] = (uint16_t)s;
        m += (u32)__builtin_popcountll(__ballot(f != 0u));
    }
    wave_sync();
    bgzf::enc_build_lengths(w, freq, n, m, limit, len, complete);
    wave_sync();
    bgzf::enc_assign_codes(w, len, n, code);
    wave_sync();
}

// The bit stream of a block on its way into its slot: `bits` written so far, of them `words` whole 32-bit words flushed; the rest,
// less than a word, is word 0 of the staging window.
struct EncOut {
    u32* slot;
    u32 bits, words;
};
// Every lane appends nb <= 48 bits v (0: nothing), in lane order: the bit lengths prefix-summed over the wave, every lane ORs its
// bits into the window (LDS atomics: the lanes share words), the whole words go to the slot in one store per 64, the last partial
// word moves to the window's front.
__device__ __forceinline__ void enc_emit(bgzf::EncWork* w, EncOut& e, u64 v, u32 nb, u32 lane) {
    u32 incl = nb;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 o = __shfl_up(incl, d, 64);
        if (lane >= (u32)d) incl += o;
    }
    const u32 total = uni(__shfl(incl, 63, 64));
    if (nb) {
        const u32 off = e.bits - 32u * e.words + (incl - nb);      // at most 31 + 63 * 48: word 95, and two more
        const u32 word = off >> 5, sh = off & 31u;
        const u64 lo = v << sh;
        const u32 hi = sh ? (u32)(v >> (64u - sh)) : 0u;
        atomicOr(&w->window[word], (u32)lo);
        if ((u32)(lo >> 32)) atomicOr(&w->window[word + 1u], (u32)(lo >> 32));
        if (hi) atomicOr(&w->window[word + 2u], hi);
    }
    wave_sync();
    e.bits += total;
    const u32 full = (e.bits >> 5) - e.words;                       // at most 96
    for (u32 i = lane; i < full; i += 64u) e.slot[e.words + i] = w->window[i];
    const u32 carry = w->window[full];
    wave_sync();
    w->window[lane] = lane == 0u ? carry : 0u;
    w->window[lane + 64u] = 0u;
    wave_sync();
    e.words += full;
}

// One DEFLATE block out of the `count` tokens gathered and their histograms: the codes, the header, the exact bit count; false (and
// nothing written) if the BGZF block would pass `limit` bits with it -- it is stored then.  Leaves the histograms cleared.
__device__ __forceinline__ bool enc_flush(bgzf::EncWork* w, EncOut& e, u32 count, u32 final_block, u32 limit, u32 lane) {
    w->lit_freq[256] = 1u;
    wave_sync();
    enc_build<5>(w, w->lit_freq, bgzf::ENC_LIT, 15u, w->lit_len, w->lit_code, true, lane);
    enc_build<1>(w, w->dist_freq, bgzf::ENC_DIST, 15u, w->dist_len, w->dist_code, false, lane);
    u32 first = 0, end = 0;
    u32 bits = uni(bgzf::enc_header(w, final_block, &first, &end));
    first = uni(first);
    end = uni(end);
    wave_sync();
    bits += uni(bgzf::enc_body_bits(w));
    if (e.bits + bits > limit) return false;
    for (u32 i = first; i < end; i += 64u) {
        const u32 item = i + lane < end ? w->tree[bgzf::ENC_ITEMS_AT + i + lane] : 0u;
        enc_emit(w, e, item & 0xFFFFFFu, item >> 24, lane);
    }
    for (u32 t = 0; t < count; t += 64u) {
        u64 v = 0;
        const u32 nb = t + lane < count ? bgzf::enc_token_bits(w, w->tokens[t + lane], &v) : 0u;
        enc_emit(w, e, v, nb, lane);
    }
    enc_emit(w, e, w->lit_code[256], lane == 0u ? (u32)w->lit_len[256] : 0u, lane);
    for (u32 s = lane; s < 288u; s += 64u) w->lit_freq[s] = 0u;
    if (lane < 32u) w->dist_freq[lane] = 0u;
    wave_sync();
    return true;
}

// The dynamic form of the block s[0, n) into e.  Greedy, in steps of 64 positions, a lane per position: every lane takes its hash's
// entry as the table stood before the step, then all update it (atomicMax of the position: the highest stays, whatever the order);
// a lane at or behind the cursor probes; from the cursor the lowest position with a match wins, the positions before it are
// literals, the cursor jumps behind the match.  false: the block is stored.
__device__ __forceinline__ bool enc_parse(const uint8_t* __restrict__ s, u32 n, bgzf::EncWork* w, EncOut& e, u32 lane) {
    for (u32 i = lane; i < (1u << bgzf::ENC_HASH_BITS); i += 64u) w->head[i] = 0u;
    for (u32 i = lane; i < 288u; i += 64u) w->lit_freq[i] = 0u;
    if (lane < 32u) w->dist_freq[lane] = 0u;
    w->window[lane] = 0u;
    w->window[lane + 64u] = 0u;
    wave_sync();
    const u32 limit = bgzf::enc_bit_limit(n);
    u32 count = 0, cur = 0;
    for (u32 base = 0; base < n; base += 64u) {
        const u32 p = base + lane;
        const bool hashed = p + 4u <= n;
        u32 h = 0, entry = 0;
        if (hashed) {
            h = bgzf::enc_hash(bgzf::load32(s + p));
            entry = w->head[h];
        }
        wave_sync();
        if (hashed) atomicMax(&w->head[h], p + 1u);
        u32 len = 0, dist = 0;
        if (p < n && p >= cur) len = bgzf::enc_probe(s, n, p, entry, &dist);
        u32 kind = 0, c = cur;                        // kind: 1 literal, 2 match
        for (;;) {                                    // (every round passes a match of at least 4: at most 16 rounds)
            const u64 m = __ballot(len != 0u && p >= c);
            if (m == 0ull) break;
            const u32 j = (u32)__builtin_ctzll(m);
            if (p >= c && p < base + j) kind = 1u;
            if (lane == j) kind = 2u;
            c = base + j + uni(__shfl(len, (int)j, 64));
        }
        if (p < n && p >= c) kind = 1u;
        cur = c > base + 64u ? c : base + 64u;
        const u32 t = kind == 2u ? bgzf::enc_match_token(len, dist) : kind == 1u ? (u32)s[p] : 0u;
        const u64 tm = __ballot(kind != 0u);
        if (kind) {
            u32 dsym;
            atomicAdd(&w->lit_freq[bgzf::enc_token_syms(t, &dsym)], 1u);
            if (dsym < 32u) atomicAdd(&w->dist_freq[dsym], 1u);
            w->tokens[count + lanes_below(tm)] = t;
        }
        count += (u32)__builtin_popcountll(tm);
        wave_sync();
        const bool last = base + 64u >= n;            // a DEFLATE block ends where the next step might not fit, and with the text
        if (last || count + 64u > bgzf::ENC_TOKENS) {
            if (!enc_flush(w, e, count, last ? 1u : 0u, limit, lane)) return false;
            count = 0;
        }
    }
    if (lane == 0u && (e.bits & 31u)) e.slot[e.words] = w->window[0];
    return true;
}

// Pieces [b0, b1) of the text, a workgroup (one wave) taking every gridDim.x-th: piece b coded into slot b - b0 (dynamic) or marked
// stored; pay[b] = its payload's bytes (| BZ_STORED_BIT), crc[b]; sizes (the sizing pass): sizes[b] = the block's bytes, stats[1] += stored
__global__ void __launch_bounds__(BZ_DEFLATE_THREADS)
bgzf_deflate_kernel(const uint8_t* __restrict__ text, u64 n_bytes, u32 bb, u64 b0, u64 b1, u32 stored_all, uint8_t* __restrict__ slots, u32 slot_bytes,
                    u32* __restrict__ pay, u32* __restrict__ crc, u64* __restrict__ sizes, unsigned long long* __restrict__ stats) {
    __shared__ bgzf::EncWork work;
    const u32 lane = lane_id();
    for (u64 b = b0 + blockIdx.x; b < b1; b += gridDim.x) {
        const uint8_t* s = text + b * bb;
        const u32 n = n_bytes - b * bb < bb ? (u32)(n_bytes - b * bb) : bb;
        EncOut e{reinterpret_cast<u32*>(slots + (b - b0) * slot_bytes), 0u, 0u};
        const bool dynamic = !stored_all && enc_parse(s, n, &work, e, lane);
        wave_sync();
#pragma unroll
        for (u32 q = 0; q < 4u; ++q) work.head[q * 64u + lane] = bgzf::crc_table_entry(q * 64u + lane);
        wave_sync();
        const u32 c = wave_crc32(work.head, s, n, lane);
        const u32 payload = dynamic ? (e.bits + 7u) / 8u : bgzf::enc_stored_bytes(n);
        if (lane == 0u) {
            pay[b] = payload | (dynamic ? 0u : BZ_STORED_BIT);
            crc[b] = c;
            if (sizes) {
                sizes[b] = (u64)(bgzf::HEADER_BYTES + bgzf::FOOTER_BYTES) + payload;
                if (!dynamic) atomicAdd(&stats[1], 1ull);
            }
        }
        wave_sync();
    }
}

// the EOF marker's size behind the pieces' and a zero behind it: the exclusive scan of n_pieces + 2 words leaves the image's size last
__global__ void bgzf_deflate_tail_kernel(u64* __restrict__ sizes, u64 n_pieces) {
    if (threadIdx.x == 0) {
        sizes[n_pieces] = bgzf::MIN_BLOCK;
        sizes[n_pieces + 1u] = 0;
    }
}

// byte r of block b of the image (b == n_pieces: the EOF marker), the block's bytes `size`
__device__ __forceinline__ u32 deflate_image_byte(const uint8_t* __restrict__ text, u64 n_bytes, u32 bb, u64 n_pieces, u64 b, u32 r, u32 size, u32 pay_word,
                                                 u32 crc_word, const uint8_t* __restrict__ slot) {
    if (r < 16u) return (u32)((r < 8u ? 0x0000000004088b1full : 0x000243420006ff00ull) >> (8u * (r & 7u))) & 255u;
    if (r < 18u) return ((size - 1u) >> (8u * (r - 16u))) & 255u;
    const bool eof = b == n_pieces;
    const u32 n = eof ? 0u : n_bytes - b * bb < bb ? (u32)(n_bytes - b * bb) : bb;
    if (r >= size - 8u) {
        const u32 k = r - (size - 8u);
        return ((k < 4u ? (eof ? 0u : crc_word) : n) >> (8u * (k & 3u))) & 255u;
    }
    const u32 q = r - 18u;
    if (eof) return q == 0u ? 3u : 0u;                              // an empty final block of the fixed code
    if (!(pay_word & BZ_STORED_BIT)) return slot[q];
    return bgzf::enc_stored_byte(text + b * bb, n, q);
}

// Blocks [b0, b1) of the image (off: where every block starts, the image's end last) written back to back.  A lane owns aligned
// 16-byte pieces of the output: a piece that lies whole inside the launch's bytes is one store, the pieces at its two ends are
// written byte by byte, their bytes outside the range not at all.
__global__ void __launch_bounds__(BZ_THREADS)
bgzf_deflate_copy_kernel(const uint8_t* __restrict__ text, u64 n_bytes, u32 bb, u64 n_pieces, const u64* __restrict__ off, const u32* __restrict__ pay,
                         const u32* __restrict__ crc, const uint8_t* __restrict__ slots, u32 slot_bytes, u64 slot_b0, u64 b0, u64 b1,
                         uint8_t* __restrict__ file) {
    const u64 lo = off[b0], hi = off[b1];
    const u64 a = (u64)(reinterpret_cast<uintptr_t>(file) & 15u);
    const u64 q0 = (lo + a) >> 4, q1 = (hi + a + 15u) >> 4;
    const u64 stride = (u64)gridDim.x * BZ_THREADS;
    for (u64 q = q0 + (u64)blockIdx.x * BZ_THREADS + threadIdx.x; q < q1; q += stride) {
        const u64 start = q * 16u;                                  // the piece is bytes [start - a, start - a + 16) of the image
        const u64 from = start < lo + a ? lo : start - a, to = start + 16u - a < hi ? start + 16u - a : hi;
        u64 l = b0, h = b1;                                         // the block of byte `from`: off[l] <= from < off[l + 1]
        while (h - l > 1u) {
            const u64 mid = l + (h - l) / 2u;
            if (off[mid] <= from) l = mid; else h = mid;
        }
        u64 b = l, o = off[b], next = off[b + 1u];
        u32 pw = b < n_pieces ? pay[b] : 0u, cw = b < n_pieces ? crc[b] : 0u;
        const bool whole = to - from == 16u;
        u32 w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
        for (u32 i = 0; i < 16u; ++i) {
            const u64 x = from + i;
            if (x >= to) continue;
            if (x >= next) {                                        // (a block has at least 28 bytes: one step)
                b += 1u;
                o = next;
                next = off[b + 1u];
                pw = b < n_pieces ? pay[b] : 0u;
                cw = b < n_pieces ? crc[b] : 0u;
            }
            const u32 v = deflate_image_byte(text, n_bytes, bb, n_pieces, b, (u32)(x - o), (u32)(next - o), pw, cw, slots + (b - slot_b0) * slot_bytes);
            if (!whole) {
                file[x] = (uint8_t)v;
            } else {
                const u32 sh = 8u * (i & 3u);
                if (i < 4u) w0 |= v << sh; else if (i < 8u) w1 |= v << sh; else if (i < 12u) w2 |= v << sh; else w3 |= v << sh;
            }
        }
        if (whole) *reinterpret_cast<uint4*>(file + from) = make_uint4(w0, w1, w2, w3);
    }
}

u32 grid_for(u64 items, u32 per_block, int n_cu) {
    const u64 want = (items + per_block - 1u) / per_block, cap = (u64)(n_cu > 0 ? n_cu : 256) * 16u;
    return (u32)(want < cap ? (want ? want : 1u) : cap);
}

}  // namespace

// ---- the index's working set: [stats: 256 B][candidates per unit: u32][pos: u64 (C + 1)][jump a, jump b, mark, rank: u32 (C + 1) each]
size_t bgzf_index_units_bytes(u64 n_bytes) { return 256u + align256((size_t)((n_bytes + BZ_UNIT - 1u) / BZ_UNIT) * 4u); }
size_t bgzf_index_scratch_bytes(u64 n_bytes, u64 n_candidates) {
    return bgzf_index_units_bytes(n_bytes) + align256((size_t)(n_candidates + 1u) * 8u) + 4u * align256((size_t)(n_candidates + 1u) * 4u);
}

// passes 1 and 2: the candidates counted per unit and the counts scanned; stats[2] = their number
hipError_t launch_bgzf_count_candidates(const uint8_t* file, u64 n_bytes, void* scratch, int n_cu, hipStream_t st) {
    const u64 n_units = (n_bytes + BZ_UNIT - 1u) / BZ_UNIT;
    unsigned long long* stats = static_cast<unsigned long long*>(scratch);
    u32* units = reinterpret_cast<u32*>(static_cast<char*>(scratch) + 256);
    hipError_t e = hipMemsetAsync(stats, 0, 256, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bgzf_candidates_kernel<false>, dim3(grid_for(n_units, BZ_WAVES, n_cu)), dim3(BZ_THREADS), 0, st, file, n_bytes, n_units, units,
                       (u64*)nullptr);
    hipLaunchKernelGGL(bgzf_scan_kernel<u32>, dim3(1), dim3(BZ_SCAN_THREADS), 0, st, units, n_units, stats + 2);
    return hipGetLastError();
}

// passes 3 to 6 over C candidates (the scanned unit counts in `scratch`): positions, successors, the chain marked, the marked ranked.
// Leaves stats[0] = text bytes, stats[1] = end of the last block, stats[3] = blocks, stats[5] = start of the last block.
hipError_t launch_bgzf_chain(const uint8_t* file, u64 n_bytes, void* scratch, u32 C, int n_cu, hipStream_t st) {
    const u64 n_units = (n_bytes + BZ_UNIT - 1u) / BZ_UNIT;
    char* base = static_cast<char*>(scratch);
    unsigned long long* stats = reinterpret_cast<unsigned long long*>(base);
    u32* units = reinterpret_cast<u32*>(base + 256);
    const size_t words = align256((size_t)(C + 1ull) * 4u);
    u64* pos = reinterpret_cast<u64*>(base + bgzf_index_units_bytes(n_bytes));
    u32* jump_a = reinterpret_cast<u32*>(reinterpret_cast<char*>(pos) + align256((size_t)(C + 1ull) * 8u));
    u32* jump_b = reinterpret_cast<u32*>(reinterpret_cast<char*>(jump_a) + words);
    u32* mark = reinterpret_cast<u32*>(reinterpret_cast<char*>(jump_b) + words);
    u32* rank = reinterpret_cast<u32*>(reinterpret_cast<char*>(mark) + words);
    const u32 grid = grid_for((u64)C + 1u, BZ_THREADS, n_cu);
    hipLaunchKernelGGL(bgzf_candidates_kernel<true>, dim3(grid_for(n_units, BZ_WAVES, n_cu)), dim3(BZ_THREADS), 0, st, file, n_bytes, n_units, units, pos);
    hipLaunchKernelGGL(bgzf_successor_kernel, dim3(grid), dim3(BZ_THREADS), 0, st, file, pos, C, jump_a, mark);
    for (u64 reach = 1; reach < (u64)C + 1u; reach <<= 1) {       // marked so far: the chain nodes at distance below `reach`
        hipLaunchKernelGGL(bgzf_mark_round_kernel, dim3(grid), dim3(BZ_THREADS), 0, st, jump_a, jump_b, mark, C);
        u32* t = jump_a;
        jump_a = jump_b;
        jump_b = t;
    }
    hipLaunchKernelGGL(bgzf_chain_stats_kernel, dim3(grid), dim3(BZ_THREADS), 0, st, file, pos, mark, C, rank, stats);
    hipLaunchKernelGGL(bgzf_scan_kernel<u32>, dim3(1), dim3(BZ_SCAN_THREADS), 0, st, rank, (u64)C, stats + 3);
    return hipGetLastError();
}

// pass 7: the arrays (n_blocks + 1 words each)
hipError_t launch_bgzf_write_index(const uint8_t* file, u64 n_bytes, void* scratch, u32 C, u64 n_blocks, u64 end, u64* block_offsets, u64* text_offsets,
                                   int n_cu, hipStream_t st) {
    char* base = static_cast<char*>(scratch);
    unsigned long long* stats = reinterpret_cast<unsigned long long*>(base);
    const size_t words = align256((size_t)(C + 1ull) * 4u);
    const u64* pos = reinterpret_cast<const u64*>(base + bgzf_index_units_bytes(n_bytes));
    const char* jump_a = reinterpret_cast<const char*>(pos) + align256((size_t)(C + 1ull) * 8u);
    const u32* mark = reinterpret_cast<const u32*>(jump_a + 2u * words);
    const u32* rank = reinterpret_cast<const u32*>(jump_a + 3u * words);
    hipLaunchKernelGGL(bgzf_write_index_kernel, dim3(grid_for((u64)C + 1u, BZ_THREADS, n_cu)), dim3(BZ_THREADS), 0, st, file, pos, mark, rank, C, n_blocks,
                       end, block_offsets, text_offsets);
    hipLaunchKernelGGL(bgzf_scan_kernel<u64>, dim3(1), dim3(BZ_SCAN_THREADS), 0, st, text_offsets, n_blocks + 1u, stats + 4);
    return hipGetLastError();
}

// decode, then CRC (check_crc) and the lowest bad block (first_bad: ~0 before)
hipError_t launch_bgzf_inflate(const uint8_t* file, u64 n_bytes, const u64* block_offsets, const u64* text_offsets, u64 n_blocks, u64 span, uint8_t* text,
                               u32* status, unsigned long long* first_bad, bool check_crc, hipStream_t st) {
    const u64 grid = (n_blocks + BZ_WAVES - 1u) / BZ_WAVES;
    if (grid == 0 || grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((u32)grid), dim3(BZ_THREADS), 0, st, file, n_bytes, block_offsets, text_offsets, n_blocks, span, text, status);
    hipLaunchKernelGGL(bgzf_crc_kernel, dim3((u32)grid), dim3(BZ_THREADS), 0, st, file, block_offsets, text_offsets, n_blocks, text, status, first_bad,
                       check_crc ? 1u : 0u);
    return hipGetLastError();
}

// ---- deflate.  The working set: [stats: 256 B][sizes, then offsets: u64 (n_pieces + 2)][pay: u32 (n_pieces)][crc: u32 (n_pieces)], and
// behind them one slot per piece coded at a time.  stats[0] = the image's bytes, stats[1] = the stored blocks.
namespace {
struct DeflateMeta {
    unsigned long long* stats;
    u64* off;
    u32 *pay, *crc;
    uint8_t* slots;
};
DeflateMeta deflate_meta(void* scratch, u64 n_pieces) {
    char* base = static_cast<char*>(scratch);
    DeflateMeta m;
    m.stats = reinterpret_cast<unsigned long long*>(base);
    m.off = reinterpret_cast<u64*>(base + 256);
    m.pay = reinterpret_cast<u32*>(reinterpret_cast<char*>(m.off) + align256((size_t)(n_pieces + 2u) * 8u));
    m.crc = reinterpret_cast<u32*>(reinterpret_cast<char*>(m.pay) + align256((size_t)(n_pieces + 1u) * 4u));
    m.slots = reinterpret_cast<uint8_t*>(reinterpret_cast<char*>(m.crc) + align256((size_t)(n_pieces + 1u) * 4u));
    return m;
}
}  // namespace
size_t bgzf_deflate_meta_bytes(u64 n_pieces) { return 256u + align256((size_t)(n_pieces + 2u) * 8u) + 2u * align256((size_t)(n_pieces + 1u) * 4u); }
u32 bgzf_deflate_slot_bytes(u32 block_bytes) { return bgzf::enc_slot_bytes(block_bytes); }
const void* bgzf_deflate_offsets(void* scratch) { return static_cast<char*>(scratch) + 256; }

// pieces [b0, b1) coded into the slots (slot_bytes 0: every piece stored); sizing: their sizes and the stored count are recorded too
hipError_t launch_bgzf_deflate_blocks(const uint8_t* text, u64 n_bytes, u32 block_bytes, u64 n_pieces, u64 b0, u64 b1, u32 slot_bytes, bool sizing,
                                      void* scratch, int n_cu, hipStream_t st) {
    if (b1 <= b0) return hipSuccess;
    const DeflateMeta m = deflate_meta(scratch, n_pieces);
    hipLaunchKernelGGL(bgzf_deflate_kernel, dim3(grid_for(b1 - b0, 1u, n_cu)), dim3(BZ_DEFLATE_THREADS), 0, st, text, n_bytes, block_bytes, b0, b1,
                       slot_bytes ? 0u : 1u, m.slots, slot_bytes, m.pay, m.crc, sizing ? m.off : (u64*)nullptr, m.stats);
    return hipGetLastError();
}
// the sizes of all pieces known: the offsets of the blocks, the marker's and the image's end behind them; stats[0] = the image's bytes
hipError_t launch_bgzf_deflate_offsets(u64 n_pieces, void* scratch, hipStream_t st) {
    const DeflateMeta m = deflate_meta(scratch, n_pieces);
    hipLaunchKernelGGL(bgzf_deflate_tail_kernel, dim3(1), dim3(64), 0, st, m.off, n_pieces);
    hipLaunchKernelGGL(bgzf_scan_kernel<u64>, dim3(1), dim3(BZ_SCAN_THREADS), 0, st, m.off, n_pieces + 2u, m.stats);
    return hipGetLastError();
}
// blocks [b0, b1) of the image (b1 up to n_pieces + 1: the marker) written; the slots hold the pieces from slot_b0 on
hipError_t launch_bgzf_deflate_copy(const uint8_t* text, u64 n_bytes, u32 block_bytes, u64 n_pieces, u64 slot_b0, u64 b0, u64 b1, u32 slot_bytes,
                                    void* scratch, u64 bytes_about, uint8_t* file, int n_cu, hipStream_t st) {
    if (b1 <= b0) return hipSuccess;
    const DeflateMeta m = deflate_meta(scratch, n_pieces);
    hipLaunchKernelGGL(bgzf_deflate_copy_kernel, dim3(grid_for(bytes_about / 16u + 2u, BZ_THREADS, n_cu)), dim3(BZ_THREADS), 0, st, text, n_bytes, block_bytes,
                       n_pieces, m.off, m.pay, m.crc, m.slots, slot_bytes, slot_b0, b0, b1, file);
    return hipGetLastError();
}

}  // namespace kmx
