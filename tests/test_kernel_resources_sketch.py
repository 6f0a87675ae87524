"""What hipcc reports for the kernels of kmx_sketch.hip: no scratch at all, no dynamic stack and no spilled register, vector or scalar.
The add, the lookup and the filter kernel -- two instances each, one- and two-word keys -- stay within 64 VGPRs (eight waves per
SIMD, the family's convention) and use no LDS; the merge uses none either, the stats kernel its 256 bins (1 024
bytes).  The counts DESIGN quotes (16 VGPRs for the add, 17 for the lookup, 20 for the filter; 26 and 17 for merge and stats) are
recorded here and not asserted: they are the compiler's of the day.  The figures are the ones kmers_amd/build.py keeps per translation
unit (-Rpass-analysis=kernel-resource-usage); in a tree where the library has not been built the source is compiled here for gfx950.
Resource metadata only."""
from tests.kernel_usage import check_usage, usage_lines

# kernel -> (instances, VGPRs as DESIGN 4.6.21 quotes them, for the record; the most it may use; the most LDS)
STEMS = {"sketch_add_kernel": (2, "16 / 16", 64, 0), "sketch_lookup_kernel": (2, "17 / 17", 64, 0),
         "sketch_filter_kernel": (2, "20 / 20", 64, 0), "sketch_merge_kernel": (1, "26", 64, 0), "sketch_stats_kernel": (1, "17", 64, 1024)}


def test_sketch_kernels_use_no_scratch(tmp_path):
    check_usage(STEMS, usage_lines("kmx_sketch.hip", tmp_path))
