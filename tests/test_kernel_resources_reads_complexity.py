"""What hipcc reports for the kernel of kmx_reads_complexity.hip: no scratch at all, no dynamic stack and no spilled register, vector
or scalar (the poly walks keep a mismatch count per letter and the window walk a dozen running counts, all wave-uniform: it is the
scalar file that runs short first, and a spill would show here).  It stays within 64 VGPRs -- what eight waves per SIMD, the
occupancy DESIGN 4.6.20 states, leave a wave -- and uses no LDS: the plane words of a window are ballots, the reductions DPP.  The
count DESIGN quotes (46 VGPRs) is recorded here and not asserted: it is the compiler's of the day.  The figures are the ones
kmers_amd/build.py keeps per translation unit (-Rpass-analysis=kernel-resource-usage); in a tree where the library has not been
built the source is compiled here for gfx950.  Resource metadata only."""
from tests.kernel_usage import check_usage, usage_lines

# kernel -> (instances, VGPRs as DESIGN 4.6.20 quotes them, for the record; the most it may use; the most LDS)
STEMS = {"reads_complexity_kernel": (1, 46, 64, 0)}


def test_reads_complexity_kernel_uses_no_scratch(tmp_path):
    check_usage(STEMS, usage_lines("kmx_reads_complexity.hip", tmp_path))
