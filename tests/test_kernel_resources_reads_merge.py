"""What hipcc reports for the kernels of kmx_reads_merge.hip: no scratch at all, no dynamic stack and no spilled register, vector or
scalar.  The merge kernel -- four instances: with and without quality bytes, with and without the batch written -- stays within 64
VGPRs and uses no LDS; the two plan kernels use what their block scan and block sum take (2 048 and 32 bytes).  The
counts DESIGN quotes (63 VGPRs with quality bytes and outputs, 35 to 42 for the others; 22 and 32 for the plan) are recorded here
and not asserted: they are the compiler's of the day.  The figures are the ones kmers_amd/build.py keeps per translation unit
(-Rpass-analysis=kernel-resource-usage); in a tree where the library has not been built the source is compiled here for gfx950.
Resource metadata only."""
from tests.kernel_usage import check_usage, usage_lines

# kernel -> (instances, VGPRs as DESIGN 4.6.17 quotes them, for the record; the most it may use; the most LDS)
STEMS = {"reads_merge_kernel": (4, "63 / 41 / 42 / 35", 64, 0), "reads_merge_plan_count_kernel": (1, "22", 64, 32),
         "reads_merge_plan_write_kernel": (1, "32", 64, 2048)}


def test_reads_merge_kernels_use_no_scratch(tmp_path):
    check_usage(STEMS, usage_lines("kmx_reads_merge.hip", tmp_path))
