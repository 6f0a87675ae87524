"""What hipcc reports for the kernel of kmx_reads_quality.hip: no scratch at all, no dynamic stack and no spilled register, vector or
scalar (the kernel carries a read's state between its steps in wave-uniform registers and sits close to what the scalar file holds:
a spill there shows here first).  It stays within 72 VGPRs -- what seven waves per SIMD, the occupancy DESIGN 4.6.15 states, leave a
wave -- and within the 2 KiB of LDS its weight table takes.  The counts DESIGN quotes (58 VGPRs, 104 SGPRs) are recorded here and not
asserted: they are the compiler's of the day.  The figures are the ones kmers_amd/build.py keeps per translation unit
(-Rpass-analysis=kernel-resource-usage); in a tree where the library has not been built the source is compiled here for gfx950.
Resource metadata only."""
from tests.kernel_usage import check_usage, usage_lines

# kernel -> (instances, VGPRs as DESIGN 4.6.15 quotes them, for the record; the most it may use; the most LDS)
STEMS = {"reads_quality_kernel": (1, 58, 72, 2048)}


def test_reads_quality_kernel_uses_no_scratch(tmp_path):
    check_usage(STEMS, usage_lines("kmx_reads_quality.hip", tmp_path))
