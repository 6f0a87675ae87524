"""What hipcc reports for the kernels of kmx_fastx_format.hip: no scratch at all, no dynamic stack and no spilled register.  The copy
kernel and the plan's count kernels stay within 64 VGPRs -- what eight waves per SIMD, the occupancy DESIGN 4.6.19 states for the
copy, leave a wave -- and the copy within the 16.5 KiB of LDS its staged record offsets, source starts and lengths take (eight
blocks of four waves a CU: 132 of the 160 KiB); the offsets kernels (a block scan over 256 words) likewise.  The counts DESIGN
quotes are recorded here beside each kernel and not asserted: they are the compiler's of the day.  The figures are the ones
kmers_amd/build.py keeps per translation unit (-Rpass-analysis=kernel-resource-usage); in a tree where the library has not been built
the source is compiled here for gfx950.  Resource metadata only."""
from tests.kernel_usage import check_usage, usage_lines

# kernel -> (instances: FASTQ and FASTA, VGPRs as DESIGN 4.6.19 quotes them, for the record; the most it may use; the most LDS)
STEMS = {"fastx_format_copy_kernel": (2, 59, 64, 16896), "fastx_format_count_kernel": (2, 17, 64, 64), "fastx_format_offsets_kernel": (2, 26, 64, 2048)}


def test_fastx_format_kernels_use_no_scratch(tmp_path):
    check_usage(STEMS, usage_lines("kmx_fastx_format.hip", tmp_path))
