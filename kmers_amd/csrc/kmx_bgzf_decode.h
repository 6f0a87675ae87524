// kmx_bgzf_decode.h -- the serial core of the BGZF / DEFLATE decoder: the bit reader, the DEFLATE block header and
// code-length parse, zlib's completeness rule, the table entries and decode-one-symbol-to-a-token with all its bounds checks.  Plain
// functions over pointers with no wave intrinsic in them: kmx_bgzf.hip runs them wave-uniformly over tables in LDS, and
// tests/cpp/bgzf_host_check.cpp runs the same text on the host (under a sanitizer) over tables in host memory.  Nothing here holds a
// local array: on the device everything indexed lives in the Work the caller hands in, so no kernel needs scratch.
//
// Every index is bounded where it is formed: a table index is a masked bit pattern, a symbol index is checked against the counts it
// was built from, a bit is never taken without being there.  A table entry of 0 means "no code of at most the primary width".
#pragma once
#include <stdint.h>

#include "../../include/kmx.h"

#ifdef __HIPCC__
#define BGZF_HD __host__ __device__ __forceinline__
#else
#define BGZF_HD inline
#endif
#ifdef __clang__
#define BGZF_NOUNROLL _Pragma("nounroll")
#else
#define BGZF_NOUNROLL
#endif

namespace kmx {
namespace bgzf {

constexpr uint32_t LIT_BITS = 10, DIST_BITS = 9;      // primary table widths
constexpr uint32_t MAX_LIT = 288, MAX_DIST = 32;      // symbols a code-length set may name (286 / 30 of them valid)
constexpr uint32_t HEADER_BYTES = 18, FOOTER_BYTES = 8, MIN_BLOCK = 28;

// One Huffman code: the primary table (entry = symbol << 4 | length, 0 = none), and what the canonical walk of the longer codes
// takes, as in puff.c: codes per length and the symbols in code order.
struct Code {
    uint16_t* tab;
    uint16_t* sym;
    uint16_t* count;   // [16]
    uint16_t* first;   // [16] canonical first code of a length
    uint16_t* offs;    // [16] index in `sym` of the first symbol of a length
    uint32_t bits;     // primary width
    uint32_t n_sym;    // symbols the set names (the bound of `sym`)
};

// What a wave (or the host check) keeps per block being decoded.  4.4 KiB.
struct Work {
    uint16_t lit_tab[1u << LIT_BITS];
    uint16_t dist_tab[1u << DIST_BITS];
    uint16_t lit_sym[MAX_LIT];
    uint16_t dist_sym[MAX_DIST];
    uint16_t lit_count[16], lit_first[16], lit_offs[16];
    uint16_t dist_count[16], dist_first[16], dist_offs[16];
    uint16_t cl_count[16], cl_first[16], cl_offs[16];
    uint16_t cl_sym[20];
    uint8_t lens[MAX_LIT + MAX_DIST];                // code lengths: literal/length set, then the distance set behind HLIT
    uint8_t cl_lens[20];
};

BGZF_HD Code lit_code(Work* w) { return Code{w->lit_tab, w->lit_sym, w->lit_count, w->lit_first, w->lit_offs, LIT_BITS, MAX_LIT}; }
BGZF_HD Code dist_code(Work* w) { return Code{w->dist_tab, w->dist_sym, w->dist_count, w->dist_first, w->dist_offs, DIST_BITS, MAX_DIST}; }
BGZF_HD Code cl_code(Work* w) { return Code{nullptr, w->cl_sym, w->cl_count, w->cl_first, w->cl_offs, 0u, 19u}; }

// ---- the 18 bytes htslib writes in front of a block; *size = BSIZE + 1 (p: at least 18 readable bytes)
BGZF_HD bool header_ok(const uint8_t* p, uint32_t* size) {
    const bool ok = p[0] == 0x1f && p[1] == 0x8b && p[2] == 8 && p[3] == 4 && p[10] == 6 && p[11] == 0 && p[12] == 'B' && p[13] == 'C' &&
                    p[14] == 2 && p[15] == 0;
    *size = ((uint32_t)p[16] | ((uint32_t)p[17] << 8)) + 1u;
    return ok;
}
BGZF_HD uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// ---- the bit reader: bytes [p, p + n), least significant bit first.  `cnt` bits of `buf` are valid, `pos` is the next byte to take.
// `ahead` holds the four bytes at `pos` whenever four are left: they are asked for one refill before they are used, so the decode does
// not wait for memory on every refill (prime() after whatever moves pos by hand).
struct Bits {
    const uint8_t* p;
    uint32_t n, pos, cnt;
    uint64_t buf;
    uint32_t ahead;
};
BGZF_HD uint32_t load32(const uint8_t* p) {     // (little-endian hosts and the device; any alignment)
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
BGZF_HD void prime(Bits& b) {
    if (b.pos + 4u <= b.n) b.ahead = load32(b.p + b.pos);
}
BGZF_HD Bits open_bits(const uint8_t* p, uint32_t n) {
    Bits b{p, n, 0u, 0u, 0ull, 0u};
    prime(b);
    return b;
}
BGZF_HD void refill(Bits& b) {
    while (b.cnt <= 32u && b.pos + 4u <= b.n) {    // four bytes at once while they are there: at least 33 bits afterwards
        b.buf |= (uint64_t)b.ahead << b.cnt;
        b.pos += 4u;
        b.cnt += 32u;
        prime(b);
    }
    while (b.cnt <= 56u && b.pos < b.n && b.pos + 4u > b.n) {   // the last three bytes, one at a time
        b.buf |= (uint64_t)b.p[b.pos++] << b.cnt;
        b.cnt += 8u;
    }
}
// k <= 16 bits, or false: the input ran out (nothing consumed then)
BGZF_HD bool take(Bits& b, uint32_t k, uint32_t* v) {
    if (b.cnt < k) refill(b);
    if (b.cnt < k) return false;
    *v = (uint32_t)b.buf & ((1u << k) - 1u);
    b.buf >>= k;
    b.cnt -= k;
    return true;
}
// the bytes not yet consumed, once the bit position is a whole byte: back to plain byte addressing (stored blocks)
BGZF_HD void to_bytes(Bits& b) {
    const uint32_t drop = b.cnt & 7u;
    b.buf >>= drop;
    b.cnt -= drop;
}
BGZF_HD void unread(Bits& b) {
    b.pos -= b.cnt >> 3;
    b.buf = 0;
    b.cnt = 0;
}
// the bytes of a stored block have been copied from p + pos
BGZF_HD void skip_bytes(Bits& b, uint32_t len) {
    b.pos += len;
    prime(b);
}

// ---- a code-length set -> counts, zlib's rule (inflate_table), first codes.  Serial: 15 steps.
// lens[0, n): the lengths; kind: 0 = the 19-symbol set (must be complete), 1 = literal/length or distance
BGZF_HD void count_lengths(const Code& c, const uint8_t* lens, uint32_t n) {
    for (uint32_t l = 0; l < 16u; ++l) c.count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) c.count[lens[s] & 15u] += 1u;
}
// 0, or KMX_BGZF_ST_CODESET.  Also leaves first[] and offs[].
BGZF_HD uint32_t kraft_and_first(const Code& c, uint32_t kind) {
    int32_t left = 1;
    uint32_t max_len = 0, code = 0, off = 0;
    c.first[0] = 0;
    c.offs[0] = 0;
    BGZF_NOUNROLL
    for (uint32_t l = 1; l < 16u; ++l) {
        const uint32_t n = c.count[l];
        left = 2 * left - (int32_t)n;
        if (left < 0) return KMX_BGZF_ST_CODESET;
        if (n) max_len = l;
        code <<= 1;
        c.first[l] = (uint16_t)code;
        c.offs[l] = (uint16_t)off;
        code += n;
        off += n;
    }
    if (left > 0) {
        if (kind == 0u) return KMX_BGZF_ST_CODESET;
        if (max_len > 1u) return KMX_BGZF_ST_CODESET;   // (one code of one bit, or -- a distance set -- none: zlib lets them through)
    }
    return 0;
}
BGZF_HD void clear_table(const Code& c, uint32_t lane, uint32_t lanes) {
    for (uint32_t i = lane; i < (1u << c.bits); i += lanes) c.tab[i] = 0;
}
// Symbol s of length len is the rank-th of its length: its place in code order, and -- a code within the primary width -- its
// replicated table entries.  Distinct symbols write distinct places, so the lanes of a wave may each place their own.
BGZF_HD void place_symbol(const Code& c, uint32_t s, uint32_t len, uint32_t rank) {
    if (len == 0u || len > 15u) return;
    const uint32_t at = (uint32_t)c.offs[len] + rank;
    if (at < c.n_sym) c.sym[at] = (uint16_t)s;
    if (c.tab && len <= c.bits) {
        const uint32_t code = ((uint32_t)c.first[len] + rank) & ((1u << len) - 1u);
        uint32_t rev = 0;
        for (uint32_t i = 0; i < len; ++i) rev |= ((code >> i) & 1u) << (len - 1u - i);
        const uint16_t e = (uint16_t)((s << 4) | len);
        for (uint32_t i = rev; i < (1u << c.bits); i += 1u << len) c.tab[i] = e;
    }
}

// ---- one symbol.  Returns the symbol, or 0x8000 | status.  The primary table first; a pattern with no entry there goes through the
// canonical compare per length (puff.c), at most 15 steps.  A code is consumed only if all its bits are there.
constexpr uint32_t SYM_ERR = 0x8000u;
BGZF_HD uint32_t walk_code(Bits& b, const Code& c) {
    uint32_t code = 0, first = 0, index = 0;
    BGZF_NOUNROLL
    for (uint32_t len = 1; len < 16u; ++len) {
        if (b.cnt < len) return SYM_ERR | KMX_BGZF_ST_INPUT;
        code |= (uint32_t)(b.buf >> (len - 1u)) & 1u;
        const uint32_t n = c.count[len];
        if (code < first + n) {
            const uint32_t at = index + (code - first);
            if (at >= c.n_sym) return SYM_ERR | KMX_BGZF_ST_BADCODE;
            b.buf >>= len;
            b.cnt -= len;
            return c.sym[at];
        }
        index += n;
        first = (first + n) << 1;
        code <<= 1;
    }
    return SYM_ERR | KMX_BGZF_ST_BADCODE;
}
BGZF_HD uint32_t symbol(Bits& b, const Code& c) {
    if (b.cnt < 15u) refill(b);
    if (c.tab) {
        const uint32_t e = c.tab[(uint32_t)b.buf & ((1u << c.bits) - 1u)];
        const uint32_t len = e & 15u;
        if (len != 0u) {
            if (len > b.cnt) return SYM_ERR | KMX_BGZF_ST_INPUT;
            b.buf >>= len;
            b.cnt -= len;
            return e >> 4;
        }
    }
    return walk_code(b, c);
}

// ---- a DEFLATE block header.  kind: 0 stored, 1 fixed, 2 dynamic.
BGZF_HD uint32_t block_header(Bits& b, uint32_t* final_block, uint32_t* kind) {
    uint32_t v;
    if (!take(b, 3u, &v)) return KMX_BGZF_ST_INPUT;
    *final_block = v & 1u;
    *kind = v >> 1;
    return *kind == 3u ? KMX_BGZF_ST_BTYPE : 0u;
}
// a stored block's LEN (the reader is left at its first byte, in byte addressing)
BGZF_HD uint32_t stored_header(Bits& b, uint32_t* len) {
    to_bytes(b);
    uint32_t l, nl;
    if (!take(b, 16u, &l) || !take(b, 16u, &nl)) return KMX_BGZF_ST_INPUT;
    if (l != (~nl & 0xFFFFu)) return KMX_BGZF_ST_STORED;
    unread(b);
    if (l > b.n - b.pos) return KMX_BGZF_ST_STORED;
    *len = l;
    return 0;
}
BGZF_HD void fixed_lengths(Work* w, uint32_t lane, uint32_t lanes, uint32_t* hlit, uint32_t* hdist) {
    for (uint32_t s = lane; s < MAX_LIT; s += lanes) w->lens[s] = s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : 8;
    for (uint32_t s = lane; s < MAX_DIST; s += lanes) w->lens[MAX_LIT + s] = 5;
    *hlit = MAX_LIT;
    *hdist = MAX_DIST;
}
// the dynamic header: HLIT, HDIST, HCLEN, the 19-symbol set and the HLIT + HDIST lengths it codes, into w->lens.  Serial.
BGZF_HD uint32_t dynamic_lengths(Bits& b, Work* w, uint32_t* hlit, uint32_t* hdist) {
    uint32_t v;
    if (!take(b, 14u, &v)) return KMX_BGZF_ST_INPUT;
    const uint32_t nlen = (v & 31u) + 257u, ndist = ((v >> 5) & 31u) + 1u, ncode = (v >> 10) + 4u;
    if (nlen > 286u || ndist > 30u) return KMX_BGZF_ST_COUNTS;
    for (uint32_t i = 0; i < 19u; ++i) w->cl_lens[i] = 0;
    for (uint32_t i = 0; i < ncode; ++i) {
        if (!take(b, 3u, &v)) return KMX_BGZF_ST_INPUT;
        // the order of RFC 1951, 3.2.7: 16 17 18 0, then 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 -- outwards from 8
        const uint32_t j = i - 3u;
        const uint32_t where = i < 3u ? 16u + i : j == 0u ? 0u : (j & 1u) ? 8u + (j - 1u) / 2u : 8u - j / 2u;
        w->cl_lens[where < 19u ? where : 0u] = (uint8_t)v;
    }
    const Code cl = cl_code(w);
    count_lengths(cl, w->cl_lens, 19u);
    if (kraft_and_first(cl, 0u)) return KMX_BGZF_ST_CODESET;
    for (uint32_t s = 0, l = 1; l < 8u; ++l)          // code order: by length, then by symbol
        for (uint32_t t = 0; t < 19u; ++t)
            if (w->cl_lens[t] == l && s < 19u) cl.sym[s++] = (uint16_t)t;
    const uint32_t total = nlen + ndist;
    uint32_t have = 0;
    while (have < total) {
        const uint32_t s = symbol(b, cl);
        if (s & SYM_ERR) return s & 0xFFu;
        if (s < 16u) {
            w->lens[have++] = (uint8_t)s;
            continue;
        }
        uint32_t rep, len = 0;
        if (s == 16u) {
            if (have == 0u) return KMX_BGZF_ST_REPEAT;
            len = w->lens[have - 1u];
            if (!take(b, 2u, &rep)) return KMX_BGZF_ST_INPUT;
            rep += 3u;
        } else if (s == 17u) {
            if (!take(b, 3u, &rep)) return KMX_BGZF_ST_INPUT;
            rep += 3u;
        } else {
            if (!take(b, 7u, &rep)) return KMX_BGZF_ST_INPUT;
            rep += 11u;
        }
        if (have + rep > total) return KMX_BGZF_ST_REPEAT;
        for (uint32_t i = 0; i < rep; ++i) w->lens[have++] = (uint8_t)len;
    }
    if (w->lens[256] == 0) return KMX_BGZF_ST_NO_EOB;
    *hlit = nlen;
    *hdist = ndist;
    return 0;
}

// ---- one token of the symbol loop
struct Token {
    uint32_t kind;    // 0 literal (a = the byte), 1 match (a = length, d = distance), 2 end of block, 3 error (a = status)
    uint32_t a, d;
};
BGZF_HD uint32_t length_base(uint32_t i) {       // i = symbol - 257 in [0, 29)
    return i < 8u ? 3u + i : i == 28u ? 258u : 3u + ((4u + (i & 3u)) << ((i >> 2) - 1u));
}
BGZF_HD uint32_t length_extra(uint32_t i) { return i < 8u || i == 28u ? 0u : (i >> 2) - 1u; }
BGZF_HD uint32_t dist_base(uint32_t i) {         // i in [0, 30)
    return i < 4u ? 1u + i : 1u + ((2u + (i & 1u)) << ((i >> 1) - 1u));
}
BGZF_HD uint32_t dist_extra(uint32_t i) { return i < 4u ? 0u : (i >> 1) - 1u; }

// produced: bytes of this BGZF block written so far; room: the bytes it may write in all
BGZF_HD Token next_token(Bits& b, const Code& lit, const Code& dist, uint32_t produced, uint32_t room) {
    const uint32_t s = symbol(b, lit);
    if (s & SYM_ERR) return Token{3u, s & 0xFFu, 0u};
    if (s < 256u) {
        if (produced >= room) return Token{3u, KMX_BGZF_ST_OUTPUT, 0u};
        return Token{0u, s, 0u};
    }
    if (s == 256u) return Token{2u, 0u, 0u};
    if (s > 285u) return Token{3u, KMX_BGZF_ST_SYMBOL, 0u};
    uint32_t extra, len = length_base(s - 257u);
    if (!take(b, length_extra(s - 257u), &extra)) return Token{3u, KMX_BGZF_ST_INPUT, 0u};
    len += extra;
    const uint32_t ds = symbol(b, dist);
    if (ds & SYM_ERR) return Token{3u, ds & 0xFFu, 0u};
    if (ds > 29u) return Token{3u, KMX_BGZF_ST_SYMBOL, 0u};
    uint32_t d = dist_base(ds);
    if (!take(b, dist_extra(ds), &extra)) return Token{3u, KMX_BGZF_ST_INPUT, 0u};
    d += extra;
    if (d > produced) return Token{3u, KMX_BGZF_ST_DISTANCE, 0u};
    if (len > room - produced) return Token{3u, KMX_BGZF_ST_OUTPUT, 0u};
    return Token{1u, len, d};
}

// ---- CRC-32 (reflected, 0xEDB88320) as polynomial arithmetic: the kernel takes the plain CRC of 64 pieces with a zero start value
// and joins them by multiplication with x^(8 * bytes behind the piece) modulo the polynomial.
constexpr uint32_t CRC_POLY = 0xEDB88320u;
BGZF_HD uint32_t crc_table_entry(uint32_t i) {
    for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ CRC_POLY : i >> 1;
    return i;
}
BGZF_HD uint32_t crc_mul(uint32_t a, uint32_t b) {      // a * b mod P, 32 steps (bit 31 = x^0)
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m != 0u; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
BGZF_HD uint32_t crc_x_pow_bytes(uint32_t n_bytes) {    // x^(8 n) mod P by squaring: x^8 is 1 << 23
    uint32_t r = 0x80000000u, sq = 0x00800000u;
    for (; n_bytes; n_bytes >>= 1) {
        if (n_bytes & 1u) r = crc_mul(r, sq);
        sq = crc_mul(sq, sq);
    }
    return r;
}
// the CRC-32 of the whole from the joined plain CRC of its n bytes: the start value 0xFFFFFFFF carried through n bytes, and the final complement
BGZF_HD uint32_t crc_finish(uint32_t plain, uint32_t n_bytes) { return plain ^ crc_mul(0xFFFFFFFFu, crc_x_pow_bytes(n_bytes)) ^ 0xFFFFFFFFu; }

}  // namespace bgzf
}  // namespace kmx
