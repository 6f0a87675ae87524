// kmx_fastx_format.hip -- a batch of reads laid out as a FASTQ or FASTA image on the device: kmx_fastx_format.  kmx.h has the
// definition of a record; it stands on the arrays alone, in 64-bit arithmetic.
//
// A record has up to nine SEGMENTS from four kinds of source: the marker, "+" and the newlines (constants); the name (bytes of
// the names batch, or the decimal digits of name_base + r); the bases, with a newline behind every line_width of them; the quality
// bytes (bytes of d_quals, or a fill byte).  The length of a record follows from three offset pairs (reads, names; the quality
// bytes lie as the bases do).
//
// Plan (kmx_reads_plan.h).  The count kernel sums the records' lengths per block, one block scans the partial sums and the total
// comes back to the host with the first and last offset of both batches: one round trip, all a count-only call without record
// offsets costs.  The offsets kernel computes the lengths again and writes where every record starts.
//
// Copy, built around the output as reads_copy_kernel is: a lane owns aligned 16-byte pieces of
// d_text, a block 4096 consecutive pieces (64 KiB).  One search per block for the record that holds the block's first byte; the
// block stages the offsets of the next 512 records in LDS together with what the walk needs of each: where its bases and its name
// start and how long they are.  A lane finds the first record of a piece among the staged ones (or by bisection in the global
// array behind them: 64 KiB hold up to 10 922 six-byte records) and walks on: a piece may hold the tail of one record, several
// whole records and the head of another.  Of a record the piece holds a range of positions [x0, x1); every segment is
// intersected with it.  Source bytes are assembled from aligned dword loads (load_words / merge_words: a dword is loaded only if
// it holds a byte that is copied), constants and digits are ored in byte by byte.  Every piece goes out as one 16-byte store
// except the image's partial first and last piece.  No atomics, no scratch.
#include "kmx_reads_plan.h"

namespace kmx {

namespace {

constexpr u32 FF_ITER = 16;               // pieces per lane
constexpr u32 FF_PIECES = CT * FF_ITER;   // pieces per block: 64 KiB of output
constexpr u32 FF_NS = 512;                // records staged in LDS per block

// what the walk needs of a record
struct Rec {
    u64 bsrc;   // where its bases (and quality bytes) start, in bytes from d_bases (d_quals)
    u64 nsrc;   // where its name starts behind name_skip, in bytes from the names' d_bases; without names: the number to spell
    u32 L, nl;  // bases; bytes of the name
};

// decimal digits of v, without a division (a loop, not nineteen 64-bit constants held in scalar registers)
__host__ __device__ __forceinline__ u32 dec_digits(u64 v) {
    u32 n = 1;
    u64 p = 10u;
#pragma unroll 1
    for (u32 i = 1; i < 20; ++i) {
        n += v >= p ? 1u : 0u;
        p *= 10u;   // (10^19 < 2^64: the last product is the last one compared)
    }
    return n;
}

__host__ __device__ __forceinline__ Rec rec_of(const FastxFormat& f, u64 r) {
    Rec rc;
    rc.L = read_span(f.offsets, f.read_len, r, rc.bsrc);
    if (f.has_names) {
        u64 a;
        const u32 len = read_span(f.name_offsets, f.name_len, r, a);
        const u32 skip = f.name_skip < len ? f.name_skip : len;
        rc.nsrc = a + skip;
        rc.nl = len - skip;
    } else {
        rc.nsrc = f.name_base + r;
        rc.nl = dec_digits(rc.nsrc);
    }
    return rc;
}

// sequence lines of a record (FASTA; a FASTQ record has one)
__host__ __device__ __forceinline__ u32 seq_lines(const FastxFormat& f, u32 L) {
    return f.width != 0u && L > f.width ? (L + f.width - 1u) / f.width : 1u;
}

template <bool FASTQ>
__host__ __device__ __forceinline__ u64 rec_len(const FastxFormat& f, const Rec& rc) {
    if (FASTQ) return (u64)rc.nl + 2u * (u64)rc.L + 6u;
    return (u64)rc.nl + 2u + (u64)rc.L + seq_lines(f, rc.L);
}

// ---- the plan
// partial[n_blocks + b] = the bytes of block b's records (partial[b] = their number); tail[2 .. 6) = the first and last offset of
// the reads and of the names
template <bool FASTQ>
__global__ void __launch_bounds__(CT) fastx_format_count_kernel(FastxFormat f, u64* __restrict__ partial, u64 n_blocks, u64* __restrict__ tail) {
    plan_count(
        f.n_reads, partial, n_blocks, [&f](u64 r) { return PlanRow{true, rec_len<FASTQ>(f, rec_of(f, r))}; },
        [&f, tail] {
            tail[2] = f.offsets ? f.offsets[0] : 0u;
            tail[3] = f.offsets ? f.offsets[f.n_reads] : 0u;
            tail[4] = f.has_names && f.name_offsets ? f.name_offsets[0] : 0u;
            tail[5] = f.has_names && f.name_offsets ? f.name_offsets[f.n_reads] : 0u;
        });
}

// rec_off[r] = where record r starts; rec_off[n_reads] = the total (tail[1])
template <bool FASTQ>
__global__ void __launch_bounds__(CT) fastx_format_offsets_kernel(FastxFormat f, const u64* __restrict__ partial, u64 n_blocks, const u64* __restrict__ tail,
                                                                  u64* __restrict__ rec_off) {
    __shared__ u64 sh[CT];
    const u64 i0 = (u64)blockIdx.x * ROWS + (u64)threadIdx.x * RPT;
    u64 len[RPT], bytes = 0;
#pragma unroll
    for (u32 j = 0; j < RPT; ++j) {
        len[j] = i0 + j < f.n_reads ? rec_len<FASTQ>(f, rec_of(f, i0 + j)) : 0u;
        bytes += len[j];
    }
    u64 tot;
    u64 b = partial[n_blocks + blockIdx.x] + block_exscan(bytes, sh, &tot);
#pragma unroll
    for (u32 j = 0; j < RPT; ++j) {
        if (i0 + j < f.n_reads) rec_off[i0 + j] = b;
        b += len[j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) rec_off[f.n_reads] = tail[1];
}

// ---- the copy
// the offsets and sources of records j0 .. j0 + cnt staged (LDS), the rest in global memory
struct Recs {
    const u64* off;            // n_reads + 1 words
    const u64 *soff, *sb, *sn; // soff[i] = off[j0 + i], i <= cnt; the Rec of record j0 + i, i < cnt, in four arrays
    const u32 *sl, *snl;
    u64 j0, n;
    u32 cnt;
    __host__ __device__ __forceinline__ u64 off_at(u64 j) const {
        const u64 d = j - j0;
        return d <= cnt ? soff[d] : off[j];
    }
    __host__ __device__ __forceinline__ Rec rec_at(const FastxFormat& f, u64 j) const {
        const u64 d = j - j0;
        return d < cnt ? Rec{sb[d], sn[d], sl[d], snl[d]} : rec_of(f, j);
    }
    // the last record j with off[j] <= ps, for j0's byte <= ps < n_bytes: bisection in the staged part, behind it in global memory
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
        u64 l = j0 + cnt, h = n;   // off[j0 + cnt] <= ps < off[n]
        while (h - l > 1u) {
            const u64 mid = (l + h) >> 1;
            if (off[mid] <= ps) l = mid;
            else h = mid;
        }
        return l;
    }
};

// byte c to byte b (0 .. 15) of the piece
__host__ __device__ __forceinline__ void put_byte(u32 (&d)[4], u32 b, u32 c) {
    const u32 v = c << (8u * (b & 3u));
#pragma unroll
    for (u32 i = 0; i < 4; ++i) d[i] |= (b >> 2) == i ? v : 0u;
}
// n copies of byte c from byte b0 of the piece on
__host__ __device__ __forceinline__ void put_fill(u32 (&d)[4], u32 b0, u32 n, u32 c) {
    const u32 m16 = ((1u << n) - 1u) << b0;
#pragma unroll
    for (u32 i = 0; i < 4; ++i) {
        const u32 nib = (m16 >> (4u * i)) & 15u;
        d[i] |= ((nib | (nib << 7) | (nib << 14) | (nib << 21)) & 0x01010101u) * c;
    }
}
// the n bytes at base + s to byte b0 of the piece on
__host__ __device__ __forceinline__ void put_bytes(u32 (&d)[4], const uint8_t* base, u64 s, u32 n, u32 b0) {
    const u32 phase = (u32)(reinterpret_cast<uintptr_t>(base) & 3u);
    u32 w[5];
    load_words(w, base, phase, s, n, b0);
    merge_words(d, w, phase, s, n, b0);
}
// digits [k0, k1) (counted from the left) of the nd decimal digits of v to byte b0 of the piece on: the number is taken apart from
// the right, by divisions by the constant 10
__host__ __device__ __forceinline__ void put_digits(u32 (&d)[4], u64 v, u32 nd, u32 k0, u32 k1, u32 b0) {
#pragma unroll 1
    for (u32 i = nd; i-- > k0;) {
        const u64 q = v / 10u;
        if (i < k1) put_byte(d, b0 + (i - k0), '0' + (u32)(v - 10u * q));
        v = q;
    }
}

// Bytes [x0, x1) of record rc (x1 - x0 <= 16) to byte b0 of the piece on.  The record, by position: marker; name [1, 1 + nl); '\n';
// the sequence lines, L + lines bytes; FASTQ: '+', '\n', the L quality bytes, '\n'.
template <bool FASTQ>
__host__ __device__ __forceinline__ void put_record(u32 (&d)[4], const FastxFormat& f, const Rec& rc, u64 x0, u64 x1, u32 b0) {
    auto at = [x0, b0](u64 x) { return b0 + (u32)(x - x0); };
    auto in = [x0, x1](u64 x) { return x >= x0 && x < x1; };
    auto lo = [x0](u64 a) { return a > x0 ? a : x0; };
    auto hi = [x1](u64 a) { return a < x1 ? a : x1; };
    if (x0 == 0u) put_byte(d, b0, FASTQ ? '@' : '>');
    const u64 n_end = 1u + (u64)rc.nl;   // the newline behind the name
    if (lo(1u) < hi(n_end)) {
        const u64 s = lo(1u), e = hi(n_end);
        if (f.has_names) put_bytes(d, f.names, rc.nsrc + (s - 1u), (u32)(e - s), at(s));
        else put_digits(d, rc.nsrc, rc.nl, (u32)(s - 1u), (u32)(e - 1u), at(s));
    }
    if (in(n_end)) put_byte(d, at(n_end), '\n');
    const u64 b_beg = n_end + 1u;
    const u64 b_end = b_beg + rc.L + (FASTQ ? 1u : seq_lines(f, rc.L));   // behind the newline that ends the last sequence line
    if (lo(b_beg) < hi(b_end)) {
        const u64 s = lo(b_beg), e = hi(b_end);
        u32 y = (u32)(s - b_beg), b = at(s);
        const u32 y1 = (u32)(e - b_beg);   // (L + lines < 2^32)
        if (FASTQ) {
            if (y < rc.L) put_bytes(d, f.bases, rc.bsrc + y, (y1 < rc.L ? y1 : rc.L) - y, b);
            if (y1 > rc.L) put_byte(d, b + (rc.L - y), '\n');
        } else {
            // position y of the lines is line y / (W + 1), column y mod (W + 1); a column W, or the end of the bases, is a newline
            const u32 W = f.width != 0u && f.width < 0x7FFFFFFFu ? f.width : 0x7FFFFFFFu;
            u32 line = 0, col = y;
            if (y > W) {
                line = y / (W + 1u);
                col = y - line * (W + 1u);
            }
#pragma unroll 1
            while (y < y1) {
                const u32 idx = line * W + col, rem = rc.L - idx;
                if (col == W || rem == 0u) {
                    put_byte(d, b, '\n');
                    ++y, ++b, ++line, col = 0;
                } else {
                    u32 n = W - col < rem ? W - col : rem;
                    n = n < y1 - y ? n : y1 - y;
                    put_bytes(d, f.bases, rc.bsrc + idx, n, b);
                    y += n, b += n, col += n;
                }
            }
        }
    }
    if (FASTQ) {
        if (in(b_end)) put_byte(d, at(b_end), '+');
        if (in(b_end + 1u)) put_byte(d, at(b_end + 1u), '\n');
        const u64 q_beg = b_end + 2u, q_end = q_beg + rc.L;
        if (lo(q_beg) < hi(q_end)) {
            const u64 s = lo(q_beg), e = hi(q_end);
            if (f.quals) put_bytes(d, f.quals, rc.bsrc + (s - q_beg), (u32)(e - s), at(s));
            else put_fill(d, at(s), (u32)(e - s), f.fill);
        }
        if (in(q_end)) put_byte(d, at(q_end), '\n');
    }
}

// Piece q of the output grid (16 q - A .. 16 q - A + 16 in output bytes, A = the address of `out` mod 16, q below the number of
// pieces): its first record found (the staged offsets below the block's end are soff[0 .. n_hi): a search of fixed steps), its
// bytes assembled record by record, stored.
template <bool FASTQ>
__host__ __device__ __forceinline__ void format_piece(const FastxFormat& f, const Recs& rd, u32 n_hi, u64 n_bytes, u64 A, u64 q, uint8_t* out) {
    const u64 pb = q * 16u;                                      // the piece's first byte, counted from out - A
    const u64 ps = pb >= A ? pb - A : 0u;                        // its output bytes [ps, pe), ps < pe
    const u64 pe = pb + 16u - A < n_bytes ? pb + 16u - A : n_bytes;
    u32 top = 1u, l = 0u;
    while (2u * top < n_hi) top *= 2u;                           // the largest power of two below n_hi (n_hi >= 1)
    for (u32 st = n_hi > 1u ? top : 0u; st != 0u; st >>= 1) {
        const u32 mid = l + st;
        if (mid < n_hi && rd.soff[mid] <= ps) l = mid;
    }
    // l == cnt: the record may lie behind the staged ones (cnt == FF_NS then: otherwise soff[cnt] = n_bytes, above every byte)
    u64 j = l == rd.cnt ? rd.find(ps) : rd.j0 + l;
    u32 d[4] = {0u, 0u, 0u, 0u};
    u64 cur = ps, o_lo = rd.off_at(j);
#pragma unroll 1
    while (cur < pe) {      // (off[n] = n_bytes >= pe: j stays below n)
        const u64 o_hi = rd.off_at(j + 1u);
        const u64 end = o_hi < pe ? o_hi : pe;
        if (end > cur) {
            put_record<FASTQ>(d, f, rd.rec_at(f, j), cur - o_lo, end - o_lo, (u32)(cur + A - pb));
            cur = end;
        }
        if (cur < pe) {
            ++j;
            o_lo = o_hi;
        }
    }
    store_piece(out + ps, d, (u32)(ps + A - pb), (u32)(pe - ps));
}

// out[0 .. n_bytes) = the records back to back (n_bytes >= 1)
template <bool FASTQ>
__global__ void __launch_bounds__(CT) fastx_format_copy_kernel(FastxFormat f, const u64* __restrict__ off, u64 n_bytes, uint8_t* __restrict__ out) {
    __shared__ u64 soff[FF_NS + 1];
    __shared__ u64 sb[FF_NS], sn[FF_NS];
    __shared__ u32 sl[FF_NS], snl[FF_NS];
    const u64 A = (u64)(reinterpret_cast<uintptr_t>(out) & 15u);   // the piece grid is the output's 16-byte grid
    const u64 n_pieces = (A + n_bytes + 15u) >> 4;
    const u64 q0 = (u64)blockIdx.x * FF_PIECES;                    // (q0 < n_pieces: the grid is sized so)
    const u64 p0 = q0 * 16u >= A ? q0 * 16u - A : 0u;              // the block's first output byte, p0 < n_bytes
    const u64 p_end = (q0 + FF_PIECES) * 16u - A < n_bytes ? (q0 + FF_PIECES) * 16u - A : n_bytes;   // behind its last
    BlockSearch bs{0u, f.n_reads};
    while (!bs.done()) {                                           // (lo and hi are the same in every thread)
        const u64 i = bs.at(threadIdx.x);
        bs.take((u64)__syncthreads_count(i < bs.hi && off[i] <= p0));
    }
    const u64 j0 = bs.lo;
    const u32 cnt = (u32)(f.n_reads - j0 < FF_NS ? f.n_reads - j0 : FF_NS);
    for (u32 i = threadIdx.x; i <= cnt; i += CT) soff[i] = off[j0 + i];
    for (u32 i = threadIdx.x; i < cnt; i += CT) {
        const Rec rc = rec_of(f, j0 + i);
        sb[i] = rc.bsrc;
        sn[i] = rc.nsrc;
        sl[i] = rc.L;
        snl[i] = rc.nl;
    }
    __syncthreads();
    // the staged offsets that are below p_end, the first included: a prefix, soff[0 .. n_hi)
    u32 n_hi = 0;
    for (u32 i0 = 0; i0 <= cnt; i0 += CT) n_hi += (u32)__syncthreads_count(i0 + threadIdx.x <= cnt && soff[i0 + threadIdx.x] < p_end);
    const Recs rd{off, soff, sb, sn, sl, snl, j0, f.n_reads, cnt};
#pragma unroll 1
    for (u32 it = 0; it < FF_ITER; ++it) {
        const u64 q = q0 + (u64)it * CT + threadIdx.x;
        if (q >= n_pieces) break;
        format_piece<FASTQ>(f, rd, n_hi, n_bytes, A, q, out);
    }
}

// the work area: the record offsets when the caller keeps none, then the plan
Plan plan_of(void* area, u64 n_reads, bool own_offsets) {
    return plan_at(static_cast<char*>(area) + (own_offsets ? align256(8u * (n_reads + 1u)) : 0u), n_reads);
}

}  // namespace

size_t fastx_format_bytes(u64 n_reads, bool own_offsets) { return (own_offsets ? align256(8u * (n_reads + 1u)) : 0u) + plan_bytes(n_reads, 6u); }

hipError_t launch_fastx_format_count(const FastxFormat& f, void* area, bool own_offsets, unsigned long long* h_pinned, u64* h_out, hipStream_t st) {
    const Plan p = plan_of(area, f.n_reads, own_offsets);
    if (f.fastq) hipLaunchKernelGGL(fastx_format_count_kernel<true>, dim3((unsigned)p.n_blocks), dim3(CT), 0, st, f, p.partial, p.n_blocks, p.tail);
    else hipLaunchKernelGGL(fastx_format_count_kernel<false>, dim3((unsigned)p.n_blocks), dim3(CT), 0, st, f, p.partial, p.n_blocks, p.tail);
    return plan_totals(p, 6u, h_pinned, h_out, st);
}

hipError_t launch_fastx_format_emit(const FastxFormat& f, void* area, bool own_offsets, u64* rec_offsets, u64 n_bytes, uint8_t* text, hipStream_t st) {
    const Plan p = plan_of(area, f.n_reads, own_offsets);
    u64* const off = own_offsets ? static_cast<u64*>(area) : rec_offsets;
    const dim3 grid((unsigned)p.n_blocks);
    if (f.fastq) hipLaunchKernelGGL(fastx_format_offsets_kernel<true>, grid, dim3(CT), 0, st, f, p.partial, p.n_blocks, p.tail, off);
    else hipLaunchKernelGGL(fastx_format_offsets_kernel<false>, grid, dim3(CT), 0, st, f, p.partial, p.n_blocks, p.tail, off);
    if (text && n_bytes != 0) {
        const u64 pieces = (((u64)reinterpret_cast<uintptr_t>(text) & 15u) + n_bytes + 15u) >> 4;
        const dim3 cgrid((unsigned)ceil_div(pieces, (u64)FF_PIECES));
        if (f.fastq) hipLaunchKernelGGL(fastx_format_copy_kernel<true>, cgrid, dim3(CT), 0, st, f, off, n_bytes, text);
        else hipLaunchKernelGGL(fastx_format_copy_kernel<false>, cgrid, dim3(CT), 0, st, f, off, n_bytes, text);
    }
    return hipGetLastError();
}

}  // namespace kmx
