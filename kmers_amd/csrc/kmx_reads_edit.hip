// kmx_reads_edit.hip -- a new ragged batch of reads from an old one: kmx_reads_select (keep, drop and clip reads) and
// kmx_reads_gather (reorder, repeat and clip them).  kmx.h has the rule of a read's span; it is defined on the arrays alone.
//
// A ROW is a source read (select) or an entry of the index (gather); a row has a CLIP -- where its bytes start in d_bases and how
// many there are -- and is kept or not.  A thread plans eight consecutive rows, a block 2048.
//
// Plan (its prologue is kmx_reads_plan.h's, the span of a read kmx_reads_common.h's).  The count kernel sums the kept rows and their
// bytes per block; one block scans the two arrays of partial sums (the count family's scan_single_kernel) and the two totals come
// back to the host with the batch's first and last offset: one round trip, all a count-only call costs.  The write kernel
// computes the clips again -- 16 bytes of offsets, a span word and a keep byte per row, cheaper than an array that carries them --
// scans kept rows and bytes over the block and writes, per OUTPUT read, its output offset, its source index (optional) and into
// the work buffer its source start.  The length of an output read is the difference of its output offsets.
//
// Copy.  Built around the output: a lane owns aligned 16-byte pieces of d_out_bases, a block 4096 consecutive
// pieces (64 KiB; a wave's 64 lanes store 1 KiB contiguous, sixteen times).  One search per block: the output read that holds the
// block's first byte, found by all 256 threads at once (each probes one of 256 evenly spaced offsets, the count of probes at or
// below the byte narrows the range 256-fold per round: three rounds for 2^24 reads).  The block then stages the offsets and source
// starts of the next 1024 output reads in LDS and counts those that begin inside its 64 KiB; a lane finds the first read of a piece
// among them by a search of fixed steps -- or, where reads are so short that 64 KiB hold more than 1024 of them, by bisection in
// the global array behind the staged part -- and walks on from it: with short reads a piece holds several reads, and runs of
// empty reads are stepped over.  The bytes of each read in the piece are assembled from ALIGNED dword loads: up to five dwords
// cover the 16 bytes at any source alignment, a funnel shift by the source's byte phase lines them up with the piece and a byte
// mask merges them.  A dword is loaded only if it holds at least one byte of the clip being copied, so the kernel never reads a
// dword that lies outside the kept clips.  Every piece is stored with one 16-byte store except the batch's first and last piece
// where they are partial: those go out byte by byte, so no byte outside [0, n_bases) is written.  Everything is unrolled over
// registers: no scratch, no atomics; 16 KiB of LDS per block, eight waves per SIMD.  (A variant that searched and loaded a lane's
// four pieces together -- 122 VGPRs, four waves -- measured 40 % slower: what hides the latency here is the waves in flight.)
#include "kmx_reads_plan.h"

namespace kmx {

namespace {

constexpr u32 CP_ITER = 16;            // pieces per lane
constexpr u32 CP_PIECES = CT * CP_ITER;   // pieces per block: 64 KiB of output
constexpr u32 CP_NS = 1024;            // output reads staged in LDS per block

struct Clip {
    u64 src;    // where the clip starts, in bytes from d_bases
    u64 len;    // 0 for a row that is not kept
    bool kept;
};

// the clip of row `row` (kmx.h, THE SPAN OF A READ): 64-bit arithmetic throughout, any bytes give one answer
template <bool GATHER>
__host__ __device__ __forceinline__ Clip clip_of(const ReadsEdit& e, u64 row) {
    u64 r = row;
    if (GATHER) {
        r = e.index[row];
        if (r >= e.n_reads) return Clip{0u, 0u, true};   // an empty read
    }
    u64 a;
    const u64 L = read_span(e.offsets, e.read_len, r, a);
    u64 start = 0u, len = L;
    if (e.span) {
        const u64 w = e.span[r * e.span_stride];
        start = w & 0xFFFFFFFFull;
        len = w >> 32;
        if (e.span_k != 0u && len != 0u) len += (u64)e.span_k - 1u;
        if (start >= L) {
            start = 0u;
            len = 0u;
        } else if (len > L - start) {
            len = L - start;
        }
    }
    const bool kept = (GATHER || !e.keep || e.keep[r] != 0u) && len >= e.min_len;
    return Clip{a + start, kept ? len : 0u, kept};
}

// partial[b] = kept rows of block b, partial[n_blocks + b] = their bytes; tail[2], tail[3] = the batch's first and last offset
template <bool GATHER>
__global__ void __launch_bounds__(CT) reads_plan_count_kernel(ReadsEdit e, u64* __restrict__ partial, u64 n_blocks, u64* __restrict__ tail) {
    plan_count(
        e.n_rows, partial, n_blocks,
        [&e](u64 row) {
            const Clip c = clip_of<GATHER>(e, row);
            return PlanRow{c.kept, c.len};
        },
        [&e, tail] {
            tail[2] = e.offsets && e.n_reads ? e.offsets[0] : 0u;
            tail[3] = e.offsets && e.n_reads ? e.offsets[e.n_reads] : 0u;
        });
}

// per output read o: out_offsets[o], src[o], out_index[o]; out_offsets[n_out] = n_bases (tail[0], tail[1]: the scanned totals)
template <bool GATHER>
__global__ void __launch_bounds__(CT) reads_plan_write_kernel(ReadsEdit e, const u64* __restrict__ partial, u64 n_blocks, const u64* __restrict__ tail,
                                                              u64* __restrict__ src, u64* __restrict__ out_offsets, u64* __restrict__ out_index) {
    __shared__ u64 sh[CT];
    const u64 i0 = (u64)blockIdx.x * ROWS + (u64)threadIdx.x * RPT;
    Clip c[RPT];
    u64 n = 0, bytes = 0;
#pragma unroll
    for (u32 j = 0; j < RPT; ++j) {
        c[j] = i0 + j < e.n_rows ? clip_of<GATHER>(e, i0 + j) : Clip{0u, 0u, false};
        n += c[j].kept ? 1u : 0u;
        bytes += c[j].len;
    }
    u64 tot;
    u64 o = partial[blockIdx.x] + block_exscan(n, sh, &tot);
    u64 b = partial[n_blocks + blockIdx.x] + block_exscan(bytes, sh, &tot);
#pragma unroll
    for (u32 j = 0; j < RPT; ++j) {
        if (c[j].kept) {
            out_offsets[o] = b;
            src[o] = c[j].src;
            if (out_index) out_index[o] = i0 + j;   // (the row: select's source read)
            ++o;
            b += c[j].len;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out_offsets[tail[0]] = tail[1];
}

// the offsets and source starts of output reads j0 .. j0 + cnt staged (LDS), the rest in global memory
struct OutReads {
    const u64 *off, *src;     // n_out + 1 and n_out words
    const u64 *soff, *ssrc;   // soff[i] = off[j0 + i], i <= cnt; ssrc[i] = src[j0 + i], i < cnt
    u64 j0, n_out;
    u32 cnt;
    __host__ __device__ __forceinline__ u64 off_at(u64 j) const {
        const u64 d = j - j0;
        return d <= cnt ? soff[d] : off[j];
    }
    __host__ __device__ __forceinline__ u64 src_at(u64 j) const {
        const u64 d = j - j0;
        return d < cnt ? ssrc[d] : src[j];
    }
    // the last read j with off[j] <= ps, for j0's byte <= ps < n_bases: bisection in the staged part, behind it in global memory
    __host__ __device__ __forceinline__ u64 find(u64 ps) const {
        if (soff[cnt] > ps) {   // soff[0] <= ps
            u32 l = 0, h = cnt;
            while (h - l > 1u) {
                const u32 mid = (l + h) >> 1;
                if (soff[mid] <= ps) l = mid;
                else h = mid;
            }
            return j0 + l;
        }
        u64 l = j0 + cnt, h = n_out;   // off[j0 + cnt] <= ps < off[n_out]
        while (h - l > 1u) {
            const u64 mid = (l + h) >> 1;
            if (off[mid] <= ps) l = mid;
            else h = mid;
        }
        return l;
    }
};

// Piece q of the output grid (16 q - A .. 16 q - A + 16 in output bytes, A = the address of `out` mod 16, q below the number of
// pieces): its first read found (the staged offsets below the block's end are soff[0 .. n_hi): a search of fixed steps), its bytes
// assembled read by read, stored.
__host__ __device__ __forceinline__ void copy_piece(const OutReads& rd, u32 n_hi, const uint8_t* bases, u64 n_bases, u64 A, u64 q, uint8_t* out) {
    const u32 phase = (u32)(reinterpret_cast<uintptr_t>(bases) & 3u);
    const u64 pb = q * 16u;                                      // the piece's first byte, counted from out - A
    const u64 ps = pb >= A ? pb - A : 0u;                        // its output bytes [ps, pe), ps < pe
    const u64 pe = pb + 16u - A < n_bases ? pb + 16u - A : n_bases;
    u32 top = 1u, l = 0u;
    while (2u * top < n_hi) top *= 2u;                           // the largest power of two below n_hi (n_hi >= 1)
    for (u32 st = n_hi > 1u ? top : 0u; st != 0u; st >>= 1) {
        const u32 mid = l + st;
        if (mid < n_hi && rd.soff[mid] <= ps) l = mid;
    }
    // l == cnt: the read may lie behind the staged ones (cnt == CP_NS then: otherwise soff[cnt] = n_bases, above every byte)
    u64 j = l == rd.cnt ? rd.find(ps) : rd.j0 + l;
    u32 d[4] = {0u, 0u, 0u, 0u};
    u64 cur = ps, o_lo = rd.off_at(j);
    while (cur < pe) {      // (off[n_out] = n_bases >= pe: j stays below n_out)
        const u64 o_hi = rd.off_at(j + 1u);
        const u64 end = o_hi < pe ? o_hi : pe;
        if (end > cur) {
            const u64 s = rd.src_at(j) + (cur - o_lo);
            const u32 n = (u32)(end - cur), b0 = (u32)(cur + A - pb);
            u32 w[5];
            load_words(w, bases, phase, s, n, b0);
            merge_words(d, w, phase, s, n, b0);
            cur = end;
        }
        if (cur < pe) {
            ++j;
            o_lo = o_hi;
        }
    }
    store_piece(out + ps, d, (u32)(ps + A - pb), (u32)(pe - ps));
}

// out[0 .. n_bases) = the clips of the n_out output reads back to back (n_bases >= 1, so n_out >= 1)
__global__ void __launch_bounds__(CT) reads_copy_kernel(const uint8_t* __restrict__ bases, const u64* __restrict__ off, const u64* __restrict__ src,
                                                        u64 n_out, u64 n_bases, uint8_t* __restrict__ out) {
    __shared__ u64 soff[CP_NS + 1];
    __shared__ u64 ssrc[CP_NS];
    const u64 A = (u64)(reinterpret_cast<uintptr_t>(out) & 15u);   // the piece grid is the output's 16-byte grid
    const u64 n_pieces = (A + n_bases + 15u) >> 4;
    const u64 q0 = (u64)blockIdx.x * CP_PIECES;                    // (q0 < n_pieces: the grid is sized so)
    const u64 p0 = q0 * 16u >= A ? q0 * 16u - A : 0u;              // the block's first output byte, p0 < n_bases
    const u64 p_end = (q0 + CP_PIECES) * 16u - A < n_bases ? (q0 + CP_PIECES) * 16u - A : n_bases;   // behind its last
    BlockSearch bs{0u, n_out};
    while (!bs.done()) {                                           // (lo and hi are the same in every thread)
        const u64 i = bs.at(threadIdx.x);
        bs.take((u64)__syncthreads_count(i < bs.hi && off[i] <= p0));
    }
    const u64 j0 = bs.lo;
    const u32 cnt = (u32)(n_out - j0 < CP_NS ? n_out - j0 : CP_NS);
    for (u32 i = threadIdx.x; i <= cnt; i += CT) soff[i] = off[j0 + i];
    for (u32 i = threadIdx.x; i < cnt; i += CT) ssrc[i] = src[j0 + i];
    __syncthreads();
    // the staged offsets that are below p_end, the first included: a prefix, soff[0 .. n_hi)
    u32 n_hi = 0;
    for (u32 i0 = 0; i0 <= cnt; i0 += CT) n_hi += (u32)__syncthreads_count(i0 + threadIdx.x <= cnt && soff[i0 + threadIdx.x] < p_end);
    const OutReads rd{off, src, soff, ssrc, j0, n_out, cnt};
#pragma unroll 1
    for (u32 it = 0; it < CP_ITER; ++it) {
        const u64 q = q0 + (u64)it * CT + threadIdx.x;
        if (q >= n_pieces) break;
        copy_piece(rd, n_hi, bases, n_bases, A, q, out);
    }
}

// the work area: the source start of every output read, then the plan
Plan plan_of(void* area, u64 n_rows) { return plan_at(static_cast<char*>(area) + align256(8u * n_rows), n_rows); }

}  // namespace

// the source start of every output read, then the partial sums (kept rows, bytes) of every block and four words for the host
size_t reads_edit_bytes(u64 n_rows) { return align256(8u * n_rows) + plan_bytes(n_rows, 4u); }

hipError_t launch_reads_edit_count(const ReadsEdit& e, void* area, unsigned long long* h_pinned, u64* h_out, hipStream_t st) {
    const Plan p = plan_of(area, e.n_rows);
    if (e.index) hipLaunchKernelGGL(reads_plan_count_kernel<true>, dim3((unsigned)p.n_blocks), dim3(CT), 0, st, e, p.partial, p.n_blocks, p.tail);
    else hipLaunchKernelGGL(reads_plan_count_kernel<false>, dim3((unsigned)p.n_blocks), dim3(CT), 0, st, e, p.partial, p.n_blocks, p.tail);
    return plan_totals(p, 4u, h_pinned, h_out, st);
}

hipError_t launch_reads_edit_emit(const ReadsEdit& e, void* area, u64 n_out, u64 n_bases, uint8_t* out_bases, u64* out_offsets, u64* out_index,
                                  hipStream_t st) {
    const Plan p = plan_of(area, e.n_rows);
    u64* src = static_cast<u64*>(area);
    const dim3 grid((unsigned)p.n_blocks);
    if (e.index) hipLaunchKernelGGL(reads_plan_write_kernel<true>, grid, dim3(CT), 0, st, e, p.partial, p.n_blocks, p.tail, src, out_offsets, out_index);
    else hipLaunchKernelGGL(reads_plan_write_kernel<false>, grid, dim3(CT), 0, st, e, p.partial, p.n_blocks, p.tail, src, out_offsets, out_index);
    if (n_bases != 0) {
        const u64 pieces = (((u64)reinterpret_cast<uintptr_t>(out_bases) & 15u) + n_bases + 15u) >> 4;
        hipLaunchKernelGGL(reads_copy_kernel, dim3((unsigned)ceil_div(pieces, (u64)CP_PIECES)), dim3(CT), 0, st, e.bases, out_offsets, src, n_out, n_bases,
                           out_bases);
    }
    return hipGetLastError();
}

}  // namespace kmx
