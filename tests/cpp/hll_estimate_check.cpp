// kmx::hll_estimate and kmx::hll_sketch_log2_blocks (include/kmx.hpp) on bins given on the command line: log2_regs, then 64 bins.
// Prints the estimate with 17 significant digits and the sketch size it gives; tests/test_hll_np.py compares both with the model.
#include <cstdio>
#include <cstdlib>

#include "kmx.hpp"

int main(int argc, char** argv) {
    if (argc != 66) return 2;
    const uint32_t log2_regs = uint32_t(std::strtoul(argv[1], nullptr, 10));
    uint64_t hist[64];
    for (int v = 0; v < 64; ++v) hist[v] = std::strtoull(argv[2 + v], nullptr, 10);
    const double e = kmx::hll_estimate(hist, log2_regs);
    std::printf("%.17g %u\n", e, kmx::hll_sketch_log2_blocks(e));
    return 0;
}
