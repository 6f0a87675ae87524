"""What hipcc reports for the kernels of kmx_reads_dedup.hip: no scratch at all, no dynamic stack and no spilled register, vector or
scalar.  The two wave-per-item kernels -- the key kernel and the verify kernel, four instances: singles or pairs, with and without
KMX_DD_STRAND -- stay within 64 VGPRs (eight waves per SIMD, the family's convention) and use no LDS; the two group
kernels and the fold of the summary use what their block sum and block scan take (32, 2 048 and 32 bytes).  The counts DESIGN quotes (29 VGPRs for the key kernel, 36
to 39 for the verify kernel; 12 and 44 for the groups) are recorded here and not asserted: they are the compiler's of the day.  The
figures are the ones kmers_amd/build.py keeps per translation unit (-Rpass-analysis=kernel-resource-usage); in a tree where the
library has not been built the source is compiled here for gfx950.  Resource metadata only."""
from tests.kernel_usage import check_usage, usage_lines

# kernel -> (instances, VGPRs as DESIGN 4.6.18 quotes them, for the record; the most it may use; the most LDS)
STEMS = {"reads_dedup_key_kernel": (1, "29", 64, 0), "reads_dedup_verify_kernel": (4, "38 / 39 / 36 / 37", 64, 0),
         "reads_dedup_head_count_kernel": (1, "12", 64, 32), "reads_dedup_head_write_kernel": (1, "44", 64, 2048),
         "reads_dedup_summary_kernel": (1, "-", 64, 32)}


def test_reads_dedup_kernels_use_no_scratch(tmp_path):
    check_usage(STEMS, usage_lines("kmx_reads_dedup.hip", tmp_path))
