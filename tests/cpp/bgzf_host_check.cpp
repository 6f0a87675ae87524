// bgzf_host_check.cpp -- kmers_amd/csrc/kmx_bgzf_decode.h on the host: the serial core of the device's BGZF decoder driven with one-lane
// stand-ins for what the wave does together (the table fill, the copies), over a corpus of blocks, sound and corrupted.  Compares the
// verdict of every block, and the bytes of the sound ones, with the expected ones (zlib's, written by tests/test_bgzf_host_decode.py).
// Built with -fsanitize=address,undefined: every buffer is allocated at its exact size, so an index the header forms out of bounds on
// hostile input stops the program here, on the CPU.
//
// corpus: u32 n; per entry u32 block bytes, u32 verdict (1 sound), u32 room (the bytes the index gives the block), u32 text bytes,
// the block, the text.   usage: bgzf_host_check <corpus>   exit 0: all as expected
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kmers_amd/csrc/kmx_bgzf_decode.h"

using namespace kmx::bgzf;

// the wave's build of one code, by one lane: the rank of a symbol among those of its length, serially
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

// one block: status, and its bytes in out[0, room)
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
    // the CRC as the kernel takes it: 64 pieces with a zero start value, joined by x^(8 * bytes behind)
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256u; ++i) tab[i] = crc_table_entry(i);
    const uint32_t piece = (room + 63u) / 64u;
    uint32_t joined = 0;
    for (uint32_t lane = 0; lane < 64u; ++lane) {
        const uint32_t lo = lane * piece < room ? lane * piece : room, hi = lo + piece < room ? lo + piece : room;
        uint32_t crc = 0;
        for (uint32_t i = lo; i < hi; ++i) crc = tab[(crc ^ out[i]) & 255u] ^ (crc >> 8);
        joined ^= crc_mul(crc, crc_x_pow_bytes(room - hi));
    }
    return crc_finish(joined, room) == le32(blk + n - 8u) ? 0u : (uint32_t)KMX_BGZF_ST_CRC;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> all;
    uint8_t buf[65536];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + k);
    std::fclose(f);
    if (all.size() < 4) return 2;
    size_t at = 4;
    const uint32_t n = le32(all.data());
    uint32_t wrong = 0, n_sound = 0, n_bad = 0;
    for (uint32_t e = 0; e < n; ++e) {
        if (at + 16 > all.size()) return 2;
        const uint32_t nb = le32(&all[at]), sound = le32(&all[at + 4]), room = le32(&all[at + 8]), nt = le32(&all[at + 12]);
        at += 16;
        if (at + nb + nt > all.size()) return 2;
        // exact-size copies: the sanitizer sees a read past the block or a write past the room
        uint8_t* blk = static_cast<uint8_t*>(std::malloc(nb ? nb : 1));
        uint8_t* out = static_cast<uint8_t*>(std::malloc(room ? room : 1));
        std::memcpy(blk, &all[at], nb);
        const uint32_t st = inflate_host(blk, nb, room, out);
        const bool same = (st == 0u) == (sound != 0u) && (st != 0u || (nt == room && std::memcmp(out, &all[at + nb], nt) == 0));
        if (!same) {
            std::printf("entry %u: status %u, expected %s\n", e, st, sound ? "sound" : "unsound");
            ++wrong;
        }
        (st ? n_bad : n_sound) += 1;
        std::free(blk);
        std::free(out);
        at += nb + nt;
    }
    std::printf("%u entries: %u sound, %u unsound, %u wrong\n", n, n_sound, n_bad, wrong);
    return wrong ? 1 : 0;
}
