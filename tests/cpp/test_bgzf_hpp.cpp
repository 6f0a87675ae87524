// test_bgzf_hpp.cpp -- kmx::naive_impl::bgzf_inflate and kmx::naive_impl::FastqReads(kmx::naive_impl::Bgzf{}, image) of include/kmx.hpp: a BGZF image (argv[1]) inflates to
// the text (argv[2]), byte for byte; the FASTQ reads taken from the image are the ones taken from the text; a plain-gzip image (argv[3])
// and a truncated one throw.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "kmx.hpp"

static std::string slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const std::string image = slurp(argv[1]), text = slurp(argv[2]), plain = slurp(argv[3]);
    kmx::Context& ctx = kmx::Context::instance();
    if (kmx::naive_impl::bgzf_inflate(ctx, image) != text) { std::puts("the inflated text differs"); return 1; }
    if (kmx::naive_impl::bgzf_inflate(ctx, image, false) != text) { std::puts("the inflated text differs (no CRC)"); return 1; }
    kmx::naive_impl::FastqReads a(kmx::naive_impl::Bgzf{}, image, ctx), b(text, ctx);
    if (a.reads().len() != b.reads().len() || a.reads().len() == 0 || a.reads().offsets() != b.reads().offsets() || a.quals() != b.quals() ||
        a.reads().read(3) != b.reads().read(3)) { std::puts("the reads differ"); return 1; }
    int thrown = 0;
    try { kmx::naive_impl::bgzf_inflate(ctx, plain); } catch (const std::exception&) { ++thrown; }
    try { kmx::naive_impl::bgzf_inflate(ctx, image.substr(0, image.size() - 5)); } catch (const std::exception&) { ++thrown; }
    std::string bad = image;
    bad[40] ^= 0x10;
    try { kmx::naive_impl::bgzf_inflate(ctx, bad); } catch (const std::exception&) { ++thrown; }
    if (thrown != 3) { std::printf("%d of 3 bad images threw\n", thrown); return 1; }
    std::puts("all C++ BGZF checks passed");
    return 0;
}
