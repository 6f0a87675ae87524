"""What hipcc reports for the kernels of kmx_reads_edit.hip: no scratch at all, no dynamic stack and no spilled register.  The copy
kernel and the plan's count kernels stay within 64 VGPRs -- what eight waves per SIMD, the occupancy DESIGN 4.6.14 states for the
copy, leave a wave -- and the copy within the 16.5 KiB of LDS its staged offsets and source starts take; the plan's write kernels (eight clips per
thread in registers) are held to 128 VGPRs, four waves per SIMD.  The counts DESIGN quotes are recorded here beside each kernel and
not asserted: they are the compiler's of the day.  The figures are the ones kmers_amd/build.py keeps per translation unit
(-Rpass-analysis=kernel-resource-usage); in a tree where the library has not been built the source is compiled here for gfx950.
Resource metadata only."""
from tests.kernel_usage import check_usage, usage_lines

# kernel -> (instances: select and gather, VGPRs as DESIGN 4.6.14 quotes them, for the record; the most it may use; the most LDS)
STEMS = {"reads_copy_kernel": (1, 48, 64, 16896), "reads_plan_count_kernel": (2, 22, 64, 64), "reads_plan_write_kernel": (2, 72, 128, 2048)}


def test_reads_edit_kernels_use_no_scratch(tmp_path):
    check_usage(STEMS, usage_lines("kmx_reads_edit.hip", tmp_path))
