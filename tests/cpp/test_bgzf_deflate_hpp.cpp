// test_bgzf_deflate_hpp.cpp -- kmx::naive_impl::bgzf_deflate of include/kmx.hpp: a text (argv[1]) cut every 9000 bytes compresses to the
// image the host model wrote (argv[2]), byte for byte, and with stored = true to zlib's level-0 image (argv[3]); what it writes
// inflates back to the text through kmx::naive_impl::bgzf_inflate; an empty text gives the 28-byte EOF marker; a block size out of
// range throws.
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
    const std::string text = slurp(argv[1]), want = slurp(argv[2]), stored = slurp(argv[3]);
    kmx::Context& ctx = kmx::Context::instance();
    const std::string image = kmx::naive_impl::bgzf_deflate(ctx, text, 9000);
    if (image != want) { std::puts("the image differs from the host model's"); return 1; }
    if (kmx::naive_impl::bgzf_deflate(ctx, text, 9000, true) != stored) { std::puts("the stored image differs from zlib's level 0"); return 1; }
    if (kmx::naive_impl::bgzf_inflate(ctx, image) != text) { std::puts("the image does not inflate to the text"); return 1; }
    if (kmx::naive_impl::bgzf_inflate(ctx, kmx::naive_impl::bgzf_deflate(ctx, text)) != text) { std::puts("the default block size does not round-trip"); return 1; }
    if (kmx::naive_impl::bgzf_deflate(ctx, std::string()).size() != 28) { std::puts("an empty text is not the EOF marker"); return 1; }
    int thrown = 0;
    try { kmx::naive_impl::bgzf_deflate(ctx, text, 65281); } catch (const std::exception&) { ++thrown; }
    if (thrown != 1) { std::puts("block_bytes 65281 did not throw"); return 1; }
    std::puts("all C++ BGZF deflate checks passed");
    return 0;
}
