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
#include "kmx_device.h"
#include "kmx_launch.h"
#include "kmx_bgzf_decode.h"

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
        const uint8_t* out = text + (ta - t0);
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
        const u32 want = bgzf::le32(file + uni64(boff[b + 1u]) - 8u);
        if (bgzf::crc_finish(crc, room) != want) {
            st = KMX_BGZF_ST_CRC;
            if (lane == 0u) status[b] = st;
        }
    }
    if (st != 0u && lane == 0u) atomicMin(first_bad, (unsigned long long)b);
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

}  // namespace kmx
