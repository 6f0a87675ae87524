"""What hipcc reports for the two kernels of kmx_reads_adapter.hip: no scratch at all, no dynamic stack and no spilled register,
vector or scalar (the adapter kernel indexes the adapters' plane words in its kernel arguments with a loop counter: an argument
struct copied to the stack would show here first).  Both stay within 64 VGPRs -- what eight waves per SIMD, the occupancy DESIGN
4.6.16 states, leave a wave; the adapter kernel uses no LDS, the pair kernel the 3 456 bytes of its plane words (four waves x two
mates x three planes x 18 words), within 4 KiB.  The counts DESIGN quotes (28 and 48 VGPRs) are recorded here and not asserted: they
are the compiler's of the day.  The figures are the ones kmers_amd/build.py keeps per translation unit
(-Rpass-analysis=kernel-resource-usage); in a tree where the library has not been built the source is compiled here for gfx950.
Resource metadata only."""
from tests.kernel_usage import check_usage, usage_lines

# kernel -> (instances, VGPRs as DESIGN 4.6.16 quotes them, for the record; the most it may use; the most LDS)
STEMS = {"reads_adapter_kernel": (1, 28, 64, 0), "reads_pair_overlap_kernel": (1, 48, 64, 4096)}


def test_reads_adapter_kernels_use_no_scratch(tmp_path):
    check_usage(STEMS, usage_lines("kmx_reads_adapter.hip", tmp_path))
