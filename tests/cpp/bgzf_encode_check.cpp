// bgzf_encode_check.cpp -- kmers_amd/csrc/kmx_bgzf_encode.h on the host: the serial core of the device's BGZF encoder driven in the
// wave's step semantics (64 positions read the hash table before any of them updates it; the highest position wins an entry; the
// lowest position with a match wins the cursor), every block decoded again with the project's host decoder (kmx_bgzf_decode.h) and
// compared with its text.  This program is the host model of kmx_bgzf_deflate: the device's image is held to its bytes.
// Built with -fsanitize=address,undefined: every text piece and every work area is allocated at its exact size.
//
// corpus: u32 n; per entry u32 block_bytes (0: 65280), u32 flags (KMX_BGZF_DEFLATE_*), u32 text bytes, the text.
// images: u32 n; per entry u32 image bytes, u32 stored blocks, u32 DEFLATE blocks inside dynamic BGZF blocks, the image.
// usage: bgzf_encode_check <corpus> <images>   exit 0: every block decoded to its text
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kmers_amd/csrc/kmx_bgzf_decode.h"
#include "../../kmers_amd/csrc/kmx_bgzf_encode.h"

using namespace kmx::bgzf;

// ---- the decoder, as tests/cpp/bgzf_host_check.cpp drives it
static uint32_t build_code_host(const Code& c, const uint8_t* lens, uint32_t n) {
    count_lengths(c, lens, n);
    c.count[0] = 0;
    if (uint32_t st = kraft_and_first(c, 1u)) return st;
    clear_table(c, 0u, 1u);
    uint32_t seen[16] = {0};
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = lens[s] & 15u;
        if (l) place_symbol(c, s, l, seen[l]++);
    }
    return 0;
}
static uint32_t plain_crc(const uint8_t* p, uint32_t n) {      // as the kernel takes it: 64 pieces joined
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256u; ++i) tab[i] = crc_table_entry(i);
    const uint32_t piece = (n + 63u) / 64u;
    uint32_t joined = 0;
    for (uint32_t lane = 0; lane < 64u; ++lane) {
        const uint32_t lo = lane * piece < n ? lane * piece : n, hi = lo + piece < n ? lo + piece : n;
        uint32_t crc = 0;
        for (uint32_t i = lo; i < hi; ++i) crc = tab[(crc ^ p[i]) & 255u] ^ (crc >> 8);
        joined ^= crc_mul(crc, crc_x_pow_bytes(n - hi));
    }
    return crc_finish(joined, n);
}
static uint32_t inflate_host(const uint8_t* blk, uint32_t n, uint32_t room, uint8_t* out) {
    uint32_t size;
    if (n < MIN_BLOCK || n > 65536u || !header_ok(blk, &size) || size != n) return KMX_BGZF_ST_HEADER;
    if (le32(blk + n - 4u) != room) return KMX_BGZF_ST_LENGTH;
    Work* w = static_cast<Work*>(std::malloc(sizeof(Work)));
    std::memset(w, 0xA5, sizeof(Work));
    Bits bits = open_bits(blk + HEADER_BYTES, n - HEADER_BYTES - FOOTER_BYTES);
    const Code lit = lit_code(w), dist = dist_code(w);
    uint32_t produced = 0, st = 0;
    for (;;) {
        uint32_t fin = 0, kind = 0;
        if ((st = block_header(bits, &fin, &kind))) break;
        if (kind == 0u) {
            uint32_t len = 0;
            if ((st = stored_header(bits, &len))) break;
            if (len > room - produced) { st = KMX_BGZF_ST_STORED; break; }
            std::memcpy(out + produced, bits.p + bits.pos, len);
            skip_bytes(bits, len);
            produced += len;
        } else {
            uint32_t hlit = 0, hdist = 0;
            if (kind == 1u) fixed_lengths(w, 0u, 1u, &hlit, &hdist);
            else if ((st = dynamic_lengths(bits, w, &hlit, &hdist))) break;
            if ((st = build_code_host(lit, w->lens, hlit))) break;
            if ((st = build_code_host(dist, w->lens + (kind == 1u ? MAX_LIT : hlit), hdist))) break;
            for (;;) {
                const Token t = next_token(bits, lit, dist, produced, room);
                if (t.kind == 0u) {
                    out[produced++] = (uint8_t)t.a;
                } else if (t.kind == 1u) {
                    for (uint32_t i = 0; i < t.a; ++i) out[produced + i] = out[produced - t.d + (t.d >= t.a ? i : i % t.d)];
                    produced += t.a;
                } else {
                    st = t.kind == 2u ? 0u : t.a;
                    break;
                }
            }
            if (st) break;
        }
        if (fin) break;
    }
    std::free(w);
    if (st) return st;
    if (produced != room) return KMX_BGZF_ST_LENGTH;
    return plain_crc(out, room) == le32(blk + n - 8u) ? 0u : (uint32_t)KMX_BGZF_ST_CRC;
}

// ---- the encoder
struct Sink {
    std::vector<uint8_t> bytes;
    uint64_t acc = 0;
    uint32_t cnt = 0, bits = 0;
    void put(uint64_t v, uint32_t n) {          // n <= 48, cnt < 8
        acc |= v << cnt;
        cnt += n;
        bits += n;
        for (; cnt >= 8u; cnt -= 8u, acc >>= 8) bytes.push_back((uint8_t)acc);
    }
    void finish() {
        if (cnt) bytes.push_back((uint8_t)acc);
        acc = 0;
        cnt = 0;
    }
};

// the wave's build of one code: every symbol in use placed by its rank, then the serial construction
static void build_host(EncWork* w, const uint32_t* freq, uint32_t n, uint32_t limit, uint8_t* len, uint16_t* code, bool complete) {
    uint32_t m = 0;
    for (uint32_t s = 0; s < n; ++s)
        if (freq[s]) {
            w->order[enc_rank(freq, n, s)] = (uint16_t)s;
            ++m;
        }
    enc_build_lengths(w, freq, n, m, limit, len, complete);
    enc_assign_codes(w, len, n, code);
}

// one DEFLATE block out of the token buffer; false: the BGZF block has passed its bit limit (it is stored)
static bool flush_host(EncWork* w, uint32_t* count, bool final_block, Sink& sink, uint32_t limit) {
    w->lit_freq[256] = 1;
    build_host(w, w->lit_freq, ENC_LIT, 15u, w->lit_len, w->lit_code, true);
    build_host(w, w->dist_freq, ENC_DIST, 15u, w->dist_len, w->dist_code, false);
    uint32_t first = 0, end = 0;
    const uint32_t bits = enc_header(w, final_block ? 1u : 0u, &first, &end) + enc_body_bits(w);
    if (sink.bits + bits > limit) return false;
    const uint32_t before = sink.bits;
    for (uint32_t i = first; i < end; ++i) sink.put(w->tree[ENC_ITEMS_AT + i] & 0xFFFFFFu, w->tree[ENC_ITEMS_AT + i] >> 24);
    for (uint32_t t = 0; t < *count; ++t) {
        uint64_t v = 0;
        const uint32_t n = enc_token_bits(w, w->tokens[t], &v);
        sink.put(v, n);
    }
    sink.put(w->lit_code[256], w->lit_len[256]);
    if (sink.bits - before != bits) {
        std::printf("bit count %u, written %u\n", bits, sink.bits - before);
        std::exit(3);
    }
    for (uint32_t s = 0; s < 288u; ++s) w->lit_freq[s] = 0;
    for (uint32_t s = 0; s < 32u; ++s) w->dist_freq[s] = 0;
    *count = 0;
    return true;
}

// the dynamic form of s[0, n) into sink; false: stored.  *n_deflate += the DEFLATE blocks written
static bool parse_host(const uint8_t* s, uint32_t n, Sink& sink, uint32_t* n_deflate) {
    EncWork* w = static_cast<EncWork*>(std::malloc(sizeof(EncWork)));
    std::memset(w, 0xA5, sizeof(EncWork));
    for (uint32_t i = 0; i < (1u << ENC_HASH_BITS); ++i) w->head[i] = 0;
    for (uint32_t i = 0; i < 288u; ++i) w->lit_freq[i] = 0;
    for (uint32_t i = 0; i < 32u; ++i) w->dist_freq[i] = 0;
    const uint32_t limit = enc_bit_limit(n);
    uint32_t count = 0, cur = 0, made = 0;
    bool ok = true;
    for (uint32_t base = 0; base < n && ok; base += 64u) {
        uint32_t hash[64], entry[64], len[64], dist[64], kind[64];
        for (uint32_t l = 0; l < 64u; ++l) {          // every lane reads the table ...
            const uint32_t p = base + l;
            hash[l] = entry[l] = len[l] = dist[l] = kind[l] = 0;
            if (p < n && p + 4u <= n) {
                hash[l] = enc_hash(load32(s + p));
                entry[l] = w->head[hash[l]];
            }
        }
        for (uint32_t l = 0; l < 64u; ++l) {          // ... before any updates it: the highest position stays
            const uint32_t p = base + l;
            if (p < n && p + 4u <= n && w->head[hash[l]] < p + 1u) w->head[hash[l]] = p + 1u;
        }
        for (uint32_t l = 0; l < 64u; ++l) {
            const uint32_t p = base + l;
            if (p < n && p >= cur) len[l] = enc_probe(s, n, p, entry[l], &dist[l]);
        }
        uint32_t c = cur;
        for (;;) {                                    // the lowest position at or behind the cursor with a match
            uint32_t j = 64;
            for (uint32_t l = 0; l < 64u; ++l)
                if (len[l] != 0u && base + l >= c) {
                    j = l;
                    break;
                }
            if (j == 64u) break;
            for (uint32_t l = 0; l < j; ++l)
                if (base + l >= c) kind[l] = 1;
            kind[j] = 2;
            c = base + j + len[j];
        }
        for (uint32_t l = 0; l < 64u; ++l)
            if (base + l < n && base + l >= c) kind[l] = 1;
        cur = c > base + 64u ? c : base + 64u;
        for (uint32_t l = 0; l < 64u; ++l) {
            if (!kind[l]) continue;
            const uint32_t t = kind[l] == 1u ? (uint32_t)s[base + l] : enc_match_token(len[l], dist[l]);
            uint32_t dsym;
            w->lit_freq[enc_token_syms(t, &dsym)] += 1u;
            if (dsym < 32u) w->dist_freq[dsym] += 1u;
            w->tokens[count++] = t;
        }
        const bool last = base + 64u >= n;            // a DEFLATE block ends where the next step might not fit, and with the text
        if (last || count + 64u > ENC_TOKENS) {
            if ((ok = flush_host(w, &count, last, sink, limit))) ++made;
        }
    }
    std::free(w);
    if (ok) {
        sink.finish();
        *n_deflate += made;
    }
    return ok;
}

static void put16(std::vector<uint8_t>& v, uint32_t x) { v.push_back((uint8_t)x), v.push_back((uint8_t)(x >> 8)); }
static void put32(std::vector<uint8_t>& v, uint32_t x) { put16(v, x & 0xFFFFu), put16(v, x >> 16); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> all;
    static uint8_t buf[65536];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + k);
    std::fclose(f);
    if (all.size() < 4) return 2;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    static const uint8_t kHead[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    static const uint8_t kEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    size_t at = 4;
    const uint32_t n_entries = le32(all.data());
    std::fwrite(all.data(), 1, 4, o);
    uint32_t wrong = 0, blocks = 0;
    for (uint32_t e = 0; e < n_entries; ++e) {
        if (at + 12 > all.size()) return 2;
        uint32_t bb = le32(&all[at]);
        const uint32_t flags = le32(&all[at + 4]), nt = le32(&all[at + 8]);
        at += 12;
        if (at + nt > all.size() || bb > ENC_BLOCK_MAX) return 2;
        if (bb == 0u) bb = ENC_BLOCK_MAX;
        std::vector<uint8_t> image;
        uint32_t n_stored = 0, n_deflate = 0;
        for (uint32_t p = 0; p < nt; p += bb) {
            const uint32_t n = nt - p < bb ? nt - p : bb;
            uint8_t* s = static_cast<uint8_t*>(std::malloc(n));       // exact size: the sanitizer sees a read past the piece
            std::memcpy(s, &all[at + p], n);
            Sink sink;
            const bool dynamic = !(flags & KMX_BGZF_DEFLATE_STORED) && parse_host(s, n, sink, &n_deflate);
            std::vector<uint8_t> blk(kHead, kHead + 16);
            const uint32_t payload = dynamic ? (uint32_t)sink.bytes.size() : enc_stored_bytes(n);
            if (dynamic && payload >= enc_stored_bytes(n)) {
                std::printf("entry %u: a dynamic block of %u bytes for %u of text\n", e, payload, n);
                ++wrong;
            }
            put16(blk, 18u + payload + 8u - 1u);
            if (dynamic) {
                blk.insert(blk.end(), sink.bytes.begin(), sink.bytes.end());
            } else {
                for (uint32_t q = 0; q < payload; ++q) blk.push_back((uint8_t)enc_stored_byte(s, n, q));
                ++n_stored;
            }
            put32(blk, plain_crc(s, n));
            put32(blk, n);
            uint8_t* out = static_cast<uint8_t*>(std::malloc(n));
            uint8_t* exact = static_cast<uint8_t*>(std::malloc(blk.size()));
            std::memcpy(exact, blk.data(), blk.size());
            const uint32_t st = inflate_host(exact, (uint32_t)blk.size(), n, out);
            if (st != 0u || std::memcmp(out, s, n) != 0) {
                std::printf("entry %u, block at %u: status %u%s\n", e, p, st, st ? "" : ", other bytes");
                ++wrong;
            }
            std::free(exact);
            std::free(out);
            std::free(s);
            image.insert(image.end(), blk.begin(), blk.end());
            ++blocks;
        }
        image.insert(image.end(), kEof, kEof + 28);
        std::vector<uint8_t> head;
        put32(head, (uint32_t)image.size());
        put32(head, n_stored);
        put32(head, n_deflate);
        std::fwrite(head.data(), 1, head.size(), o);
        std::fwrite(image.data(), 1, image.size(), o);
        at += nt;
    }
    std::fclose(o);
    std::printf("%u entries, %u blocks, %u wrong\n", n_entries, blocks, wrong);
    return wrong ? 1 : 0;
}
