// include/kmx.hpp's SipHasher13State overloads (std's DefaultHasher / RandomState): canonical_reduce, Kmer::minimizer and
// SeqVector::iter_minimizers.  Prints what they return on a fixed batch (tests/test_cpp_sip13.py compares it with the Python path)
// and checks the property of the reference's test_minimizer (kmer.rs:560-580) itself.  Exit code 0 = all checks passed.
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

#include "kmx.hpp"

using namespace kmx;
using namespace kmx::naive_impl;

static int failures = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);       \
            ++failures;                                               \
        }                                                             \
    } while (0)

// the batch: n reads of L bases, byte i = "ACGT"[(x >> 33) & 3] of a 64-bit LCG (the Python side repeats it)
static std::string batch(size_t nbytes) {
    std::string s(nbytes, 'A');
    uint64_t x = 12345;
    for (size_t i = 0; i < nbytes; ++i) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        s[i] = "ACGT"[(x >> 33) & 3u];
    }
    return s;
}

int main() {
    Context& ctx = Context::instance();
    const hash::SipHasher13State st{0x0706050403020100ull, 0x0F0E0D0C0B0A0908ull};
    const size_t n = 70, L = 150;
    const std::string s = batch(n * L);
    DeviceBuffer<uint8_t> d(ctx, reinterpret_cast<const uint8_t*>(s.data()), s.size());
    const kmx_reads reads{d.data(), n, static_cast<uint32_t>(L), nullptr};
    for (uint32_t flags : {0u, 1u}) {
        const kmx_summary r = canonical_reduce(ctx, reads, 31, st, flags);
        std::printf("reduce %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", flags, r.n_valid, r.sum_canon, r.xor_hash, r.sum_fw);
        const kmx_summary lex = canonical_reduce(ctx, reads, 31, KMX_HASH_NONE, 0, flags);
        CHECK(r.n_valid == lex.n_valid && r.sum_canon == lex.sum_canon && r.sum_fw == lex.sum_fw);
    }
    // SeqVector::iter_minimizers over the first read
    SeqVector sv(s.substr(0, L), ctx);
    const auto mm = sv.iter_minimizers(31, 15, st);
    for (const auto& m : mm) std::printf("mm %" PRIu64 " %zu\n", m.word, m.pos);
    // test_minimizer (kmer.rs:560-580) with a RandomState-like key pair: the chosen l-mer's hash is <= every other l-mer's hash of
    // the k-mer, and the l-mer at the offset is the minimizer
    for (size_t i = 0; i < 20; ++i) {
        const Kmer km = Kmer::from(s.substr(i * 7, 31), ctx);
        const auto [mmer, off] = km.minimizer(15, st, ctx);
        const uint64_t h = hash::hash_one(st, mmer, ctx);
        for (size_t p = 0; p + 15 <= 31; ++p) CHECK(h <= hash::hash_one(st, km.sub_kmer(p, 15), ctx));
        CHECK(km.sub_kmer(off, 15) == mmer);
        std::printf("kmer %zu %" PRIu64 " %zu\n", i, mmer.data, off);
    }
    if (failures == 0) std::printf("all sip13 C++ checks passed\n");
    return failures == 0 ? 0 : 1;
}
