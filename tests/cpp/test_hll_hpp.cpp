// kmx::Hll (include/kmx.hpp) on the GPU: the keys i * 0x9e3779b97f4a7c15 for i in [0, n) go into registers of log2_regs under `seed`,
// the first half of them into a second array, and the program prints three lines of 64 bins -- all keys, the first half, the merge of
// the two (which must be the first again) -- and a line with estimate, sketch_log2_blocks and the three numbers of compare.
// tests/test_gpu_hll.py compares them with the host model.  usage: test_hll_hpp n log2_regs seed
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kmx.hpp"

static void print_bins(const std::vector<uint64_t>& h, size_t at) {
    for (size_t v = 0; v < 64; ++v) std::printf("%llu%c", (unsigned long long)h[at + v], v == 63 ? '\n' : ' ');
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const uint64_t n = std::strtoull(argv[1], nullptr, 10), seed = std::strtoull(argv[3], nullptr, 10);
    const uint32_t log2_regs = uint32_t(std::strtoul(argv[2], nullptr, 10));
    try {
        kmx::Context ctx(0);
        std::vector<uint64_t> keys(n);
        for (uint64_t i = 0; i < n; ++i) keys[i] = i * 0x9e3779b97f4a7c15ull;
        kmx::DeviceBuffer<uint64_t> d_keys(ctx, keys.data(), n);
        kmx::Hll all(ctx, log2_regs, seed), half(ctx, log2_regs, seed);
        all.add_words(d_keys.data(), n);
        half.add_words(d_keys.data(), n / 2);
        const auto both = all.histogram(&half);
        print_bins(both, 0);
        print_bins(both, 64);
        half.merge(all);
        print_bins(half.histogram(), 0);
        const auto c = all.compare(half);
        std::printf("%.17g %u %.17g %.17g %.17g\n", all.estimate(), all.sketch_log2_blocks(), c[0], c[1], c[2]);
        bool same = true;
        for (size_t v = 0; v < 64; ++v) same = same && both[v] == both[128 + v];   // max(all, half) == all
        std::printf(same ? "all C++ hll checks passed\n" : "max(all, half) differs from all\n");
        return same ? 0 : 1;
    } catch (const kmx::Panic& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
