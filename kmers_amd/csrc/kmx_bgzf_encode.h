// kmx_bgzf_encode.h -- the serial core of the BGZF / DEFLATE encoder: the hash, the probe of one position (its table
// candidate and the distance-1 candidate, the match extended and bounded), the token form, the length / distance symbols, the
// length-limited Huffman code of a histogram, the dynamic block header with its repeat symbols, and the bits of a token.  Plain
// functions over pointers with no wave intrinsic in them, in the manner of kmx_bgzf_decode.h: kmx_bgzf.hip runs the per-position
// ones a lane per position and the code construction wave-uniformly over an EncWork in LDS, and tests/cpp/bgzf_encode_check.cpp runs
// the same text on the host (under a sanitizer) in the wave's step semantics.  Nothing here holds a local array.
//
// The bytes of a block are a function of its text alone: every rule below has one answer (ties go to the lower symbol, the leaf
// before the internal node, the distance-1 candidate before the table's).
#pragma once
#include <stdint.h>

#include "kmx_bgzf_decode.h"

namespace kmx {
namespace bgzf {

constexpr uint32_t ENC_BLOCK_MAX = 65280;             // text bytes a BGZF block takes at most (htslib's)
constexpr uint32_t ENC_HASH_BITS = 11;
constexpr uint32_t ENC_TOKENS = 4096;                 // tokens of one DEFLATE block (the end-of-block symbol not counted)
constexpr uint32_t ENC_MAX_MATCH = 258, ENC_MAX_DIST = 32768;
constexpr uint32_t ENC_LIT = 286, ENC_DIST = 30, ENC_CL = 19;
constexpr uint32_t ENC_ITEMS_AT = 64;                 // where the header items start in EncWork::tree
constexpr uint32_t ENC_ITEMS = 21 + ENC_LIT + ENC_DIST;   // 3 + 14 header bits, 19 lengths, one item per coded length at the most
constexpr uint32_t ENC_WINDOW = 128;                  // words of the staging window: 64 lanes x 48 bits = 96 words a step, and the carry
constexpr uint32_t ENC_STORED_SPLIT = 32768;          // from this many bytes on zlib's level 0 writes a non-final stored block and an empty final one

// What a wave (or the host check) keeps per BGZF block being coded.  Just under 31 KiB.
struct EncWork {
    uint32_t head[1u << ENC_HASH_BITS];   // hash -> position + 1 of the last 4 bytes with it (0: none); the CRC table once the parse is over
    uint32_t tokens[ENC_TOKENS];
    uint32_t lit_freq[288], dist_freq[32], cl_freq[20];
    uint32_t tree[2 * 288];               // node weights while a code is built (the 19-symbol code's: 37 words); the items of the header from word 64
    uint16_t parent[2 * 288];             // ... the parent of a node, then its depth
    uint16_t order[288];                  // the symbols in use, ascending by (count, symbol)
    uint16_t lit_code[288], dist_code[32], cl_code[20];   // bit-reversed
    uint16_t bl_count[16], next_code[16];
    uint8_t lit_len[288], dist_len[32], cl_len[20];
    uint32_t window[ENC_WINDOW];
};

BGZF_HD uint32_t enc_hash(uint32_t four) { return (four * 2654435761u) >> (32u - ENC_HASH_BITS); }

// bytes s[p + i] == s[p - d + i] for i < the result <= max (max <= 258, p + max inside the block, d <= p)
BGZF_HD uint32_t enc_match_len(const uint8_t* s, uint32_t p, uint32_t d, uint32_t max) {
    uint32_t l = 0;
    while (l + 4u <= max && load32(s + p + l) == load32(s + p - d + l)) l += 4u;
    while (l < max && s[p + l] == s[p - d + l]) ++l;
    return l;
}
// Is a match worth its length and distance codes?  Text that costs about two bits a byte (bases, quality runs) loses on a short far
// match: a distance of d costs log2(d) - 1 extra bits beside the two symbols.
BGZF_HD bool enc_worth(uint32_t len, uint32_t dist) {
    return len >= (dist <= 1u ? 4u : dist <= 16u ? 5u : dist <= 256u ? 6u : dist <= 4096u ? 8u : 10u);
}
// The match position p of the block s[0, n) takes, 0 for none: `entry` is its hash's table entry as it stood before the step (a
// position + 1 below p's step).  The distance-1 candidate first (runs), then the table's, if it is longer.
BGZF_HD uint32_t enc_probe(const uint8_t* s, uint32_t n, uint32_t p, uint32_t entry, uint32_t* dist) {
    const uint32_t max = n - p < ENC_MAX_MATCH ? n - p : ENC_MAX_MATCH;
    uint32_t best = 0, bd = 0;
    if (p >= 1u && max >= 4u) {
        const uint32_t l = enc_match_len(s, p, 1u, max);
        if (enc_worth(l, 1u)) best = l, bd = 1u;
    }
    if (entry != 0u && entry - 1u < p && max >= 4u) {
        const uint32_t d = p - (entry - 1u);
        if (d > 1u && d <= ENC_MAX_DIST) {
            const uint32_t l = enc_match_len(s, p, d, max);
            if (l > best && enc_worth(l, d)) best = l, bd = d;
        }
    }
    *dist = bd;
    return best;
}

// ---- tokens: a literal is its byte; a match is bit 31, the distance - 1 in bits 8..22, the length - 3 in bits 0..7
BGZF_HD uint32_t enc_match_token(uint32_t len, uint32_t dist) { return 0x80000000u | ((dist - 1u) << 8) | (len - 3u); }
BGZF_HD uint32_t enc_len_sym(uint32_t len) {          // 3..258 -> the index length_base takes, [0, 29)
    if (len == 258u) return 28u;
    const uint32_t l = len - 3u;
    if (l < 8u) return l;
    const uint32_t e = (31u - (uint32_t)__builtin_clz(l)) - 2u;
    return 4u * (e + 1u) + ((l >> e) & 3u);
}
BGZF_HD uint32_t enc_dist_sym(uint32_t dist) {        // 1..32768 -> [0, 30)
    const uint32_t x = dist - 1u;
    if (x < 4u) return x;
    const uint32_t e = (31u - (uint32_t)__builtin_clz(x)) - 1u;
    return 2u * (e + 1u) + ((x >> e) & 1u);
}
// the literal/length symbol of a token, and -- a match -- its distance symbol (else 32)
BGZF_HD uint32_t enc_token_syms(uint32_t t, uint32_t* dsym) {
    if (!(t >> 31)) {
        *dsym = 32u;
        return t & 511u;
    }
    *dsym = enc_dist_sym(((t >> 8) & 0x7FFFu) + 1u);
    return 257u + enc_len_sym((t & 255u) + 3u);
}
// the bits of a token under the codes in w, least significant first: at most 15 + 5 + 15 + 13 = 48
BGZF_HD uint32_t enc_token_bits(const EncWork* w, uint32_t t, uint64_t* v) {
    if (!(t >> 31)) {
        *v = w->lit_code[t & 511u];
        return w->lit_len[t & 511u];
    }
    const uint32_t len = (t & 255u) + 3u, dist = ((t >> 8) & 0x7FFFu) + 1u;
    const uint32_t li = enc_len_sym(len), di = enc_dist_sym(dist);
    uint64_t val = w->lit_code[257u + li];
    uint32_t n = w->lit_len[257u + li];
    val |= (uint64_t)(len - length_base(li)) << n;
    n += length_extra(li);
    val |= (uint64_t)w->dist_code[di] << n;
    n += w->dist_len[di];
    val |= (uint64_t)(dist - dist_base(di)) << n;
    n += dist_extra(di);
    *v = val;
    return n;
}

// ---- a histogram -> code lengths of at most `limit` bits
// the place of symbol s (freq[s] != 0) among the symbols in use, ascending by (count, symbol): one call per symbol fills `order`
BGZF_HD uint32_t enc_rank(const uint32_t* freq, uint32_t n, uint32_t s) {
    const uint32_t f = freq[s];
    uint32_t r = 0;
    for (uint32_t t = 0; t < n; ++t) {
        const uint32_t ft = freq[t];
        r += (ft != 0u && (ft < f || (ft == f && t < s))) ? 1u : 0u;
    }
    return r;
}
// order[0, m): the symbols in use.  Huffman's code by the two-queue merge (the leaves ascending, the internal nodes in the order they
// are made; a leaf wins a tie), the depths read off the parents.  A code deeper than `limit` is built again over the counts halved
// (rounded up, so the order stands): at the latest when every count is 1 the depth is ceil(log2 m) <= 9.  complete: the set must be
// complete (literal/length, code-length code), so a lone symbol gets a partner; a distance set may hold one code of one bit -- the
// exception zlib allows -- and with no match at all holds that one code for distance 1.
BGZF_HD void enc_build_lengths(EncWork* w, const uint32_t* freq, uint32_t n, uint32_t m, uint32_t limit, uint8_t* len, bool complete) {
    for (uint32_t s = 0; s < n; ++s) len[s] = 0;
    if (m < 2u) {
        const uint32_t s = m ? w->order[0] : 0u;
        len[s] = 1;
        if (complete) len[s == 0u ? 1u : 0u] = 1;
        return;
    }
    const uint32_t root = 2u * m - 2u;
    for (uint32_t sh = 0; sh < 32u; ++sh) {
        for (uint32_t i = 0; i < m; ++i) w->tree[i] = ((freq[w->order[i]] - 1u) >> sh) + 1u;
        uint32_t i = 0, j = m;
        for (uint32_t k = m; k <= root; ++k) {
            uint32_t a, b;
            if (i < m && (j >= k || w->tree[i] <= w->tree[j])) a = i++; else a = j++;
            if (i < m && (j >= k || w->tree[i] <= w->tree[j])) b = i++; else b = j++;
            w->tree[k] = w->tree[a] + w->tree[b];
            w->parent[a] = (uint16_t)k;
            w->parent[b] = (uint16_t)k;
        }
        w->parent[root] = 0;
        uint32_t deepest = 0;
        for (uint32_t k = root; k-- > 0u;) {              // (a parent's index is above its children's: its depth is there already)
            const uint32_t d = (uint32_t)w->parent[w->parent[k]] + 1u;
            w->parent[k] = (uint16_t)d;
            if (k < m && d > deepest) deepest = d;
        }
        if (deepest <= limit) break;
    }
    for (uint32_t i = 0; i < m; ++i) len[w->order[i]] = (uint8_t)w->parent[i];
}
// the canonical codes of a length set, bit-reversed (DEFLATE sends a code from its most significant bit)
BGZF_HD void enc_assign_codes(EncWork* w, const uint8_t* len, uint32_t n, uint16_t* code) {
    for (uint32_t l = 0; l < 16u; ++l) w->bl_count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) w->bl_count[len[s] & 15u] += 1u;
    w->bl_count[0] = 0;
    uint32_t c = 0;
    w->next_code[0] = 0;
    for (uint32_t l = 1; l < 16u; ++l) {
        c = (c + w->bl_count[l - 1u]) << 1;
        w->next_code[l] = (uint16_t)c;
    }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = len[s] & 15u;
        uint32_t rev = 0;
        if (l) {
            const uint32_t v = w->next_code[l];
            w->next_code[l] = (uint16_t)(v + 1u);
            for (uint32_t i = 0; i < l; ++i) rev |= ((v >> i) & 1u) << (l - 1u - i);
        }
        code[s] = (uint16_t)rev;
    }
}

// ---- the header of a dynamic block
// an item: its bits in the low 24, their number above
BGZF_HD uint32_t enc_item(uint32_t value, uint32_t nbits) { return (nbits << 24) | value; }
BGZF_HD uint32_t enc_cl_order(uint32_t i) {           // RFC 1951, 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    const uint32_t j = i - 3u;
    return i < 3u ? 16u + i : j == 0u ? 0u : (j & 1u) ? 8u + (j - 1u) / 2u : 8u - j / 2u;
}
BGZF_HD uint32_t enc_cl_put(EncWork* w, uint32_t k, uint32_t sym, uint32_t extra) {
    if (k < ENC_LIT + ENC_DIST) w->tree[ENC_ITEMS_AT + 21u + k] = sym | (extra << 8);
    w->cl_freq[sym] += 1u;
    return k + 1u;
}
// From lit_len / dist_len: HLIT and HDIST trimmed, the lengths run-length coded with 16 / 17 / 18 (one sequence over both sets), the
// code of those symbols (at most 7 bits, complete), and all of it as items in w->tree[ENC_ITEMS_AT + *first, ENC_ITEMS_AT + *end).
// Returns the bits of the header, the three block bits included.
BGZF_HD uint32_t enc_header(EncWork* w, uint32_t final_block, uint32_t* first, uint32_t* end) {
    uint32_t hlit = ENC_LIT, hdist = ENC_DIST;
    while (hlit > 257u && w->lit_len[hlit - 1u] == 0) --hlit;
    while (hdist > 1u && w->dist_len[hdist - 1u] == 0) --hdist;
    const uint32_t total = hlit + hdist;
    for (uint32_t c = 0; c < 20u; ++c) w->cl_freq[c] = 0;
    uint32_t k = 0;
    for (uint32_t i = 0; i < total;) {
        const uint32_t v = i < hlit ? w->lit_len[i] : w->dist_len[i - hlit];
        uint32_t run = 1;
        while (i + run < total && (i + run < hlit ? w->lit_len[i + run] : w->dist_len[i + run - hlit]) == v) ++run;
        i += run;
        if (v == 0u) {
            while (run >= 11u) {
                const uint32_t r = run < 138u ? run : 138u;
                k = enc_cl_put(w, k, 18u, r - 11u);
                run -= r;
            }
            if (run >= 3u) {
                k = enc_cl_put(w, k, 17u, run - 3u);
                run = 0;
            }
        } else {
            k = enc_cl_put(w, k, v, 0u);
            run -= 1u;
            while (run >= 3u) {
                const uint32_t r = run < 6u ? run : 6u;
                k = enc_cl_put(w, k, 16u, r - 3u);
                run -= r;
            }
        }
        for (; run; --run) k = enc_cl_put(w, k, v, 0u);
    }
    uint32_t m = 0;
    for (uint32_t c = 0; c < ENC_CL; ++c)
        if (w->cl_freq[c]) {
            w->order[enc_rank(w->cl_freq, ENC_CL, c)] = (uint16_t)c;
            ++m;
        }
    enc_build_lengths(w, w->cl_freq, ENC_CL, m, 7u, w->cl_len, true);
    enc_assign_codes(w, w->cl_len, ENC_CL, w->cl_code);
    uint32_t hclen = ENC_CL;
    while (hclen > 4u && w->cl_len[enc_cl_order(hclen - 1u)] == 0) --hclen;
    uint32_t* items = w->tree + ENC_ITEMS_AT;
    const uint32_t at = 19u - hclen;
    items[at] = enc_item((final_block & 1u) | 4u, 3u);
    items[at + 1u] = enc_item((hlit - 257u) | ((hdist - 1u) << 5) | ((hclen - 4u) << 10), 14u);
    for (uint32_t i = 0; i < hclen; ++i) items[at + 2u + i] = enc_item(w->cl_len[enc_cl_order(i)], 3u);
    uint32_t bits = 17u + 3u * hclen;
    for (uint32_t i = 0; i < k; ++i) {
        const uint32_t raw = items[21u + i], sym = raw & 31u, extra = raw >> 8;
        const uint32_t l = w->cl_len[sym], xb = sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u;
        items[21u + i] = enc_item((uint32_t)w->cl_code[sym] | (extra << l), l + xb);
        bits += l + xb;
    }
    *first = at;
    *end = 21u + k;
    return bits;
}
// the bits of the block's body under the codes in w: every counted symbol (the end-of-block symbol is counted) and its extra bits
BGZF_HD uint32_t enc_body_bits(const EncWork* w) {
    uint32_t bits = 0;
    for (uint32_t s = 0; s < ENC_LIT; ++s) bits += w->lit_freq[s] * ((uint32_t)w->lit_len[s] + (s >= 257u ? length_extra(s - 257u) : 0u));
    for (uint32_t d = 0; d < ENC_DIST; ++d) bits += w->dist_freq[d] * ((uint32_t)w->dist_len[d] + dist_extra(d));
    return bits;
}

// ---- sizes.  The stored form of n bytes is zlib's at level 0, byte for byte: one final stored block (1 + LEN + NLEN + the bytes)
// below 32768 bytes; from there on a stored block that is not final and an empty final one behind it.  A BGZF block takes the
// dynamic form iff its DEFLATE stream is shorter in whole bytes than the stored form.  A block is given up for stored as soon as its
// bits pass that, so a slot of enc_slot_bytes holds it (whole words are written: three bytes more at the most).
BGZF_HD uint32_t enc_stored_bytes(uint32_t n) { return n + (n < ENC_STORED_SPLIT ? 5u : 10u); }
// byte q of the stored form of the n bytes s
BGZF_HD uint32_t enc_stored_byte(const uint8_t* s, uint32_t n, uint32_t q) {
    if (q >= 5u && q < 5u + n) return s[q - 5u];
    if (q == 0u) return n < ENC_STORED_SPLIT ? 1u : 0u;
    if (q < 5u) return ((q < 3u ? n : ~n) >> (8u * ((q - 1u) & 1u))) & 255u;
    const uint32_t k = q - 5u - n;                     // the empty final block: 01 00 00 ff ff
    return k == 0u ? 1u : k < 3u ? 0u : 255u;
}
BGZF_HD uint32_t enc_bit_limit(uint32_t n) { return 8u * (enc_stored_bytes(n) - 1u); }
BGZF_HD uint32_t enc_slot_bytes(uint32_t block_bytes) { return (block_bytes + 16u + 255u) & ~255u; }

}  // namespace bgzf
}  // namespace kmx
