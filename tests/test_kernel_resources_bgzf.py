"""What hipcc reports for the kernels of kmx_bgzf.hip: no scratch at all, no dynamic stack and no spilled register.  The bounds are the
ones DESIGN 4.6.22 derives from the hardware table, not measured ones: the inflate kernel -- one wave per BGZF block, four waves a
workgroup -- within 128 VGPRs (four waves per SIMD) and 40 KiB of LDS per workgroup (four workgroups per CU of 160 KiB); the CRC and
index kernels within the same.  The counts DESIGN quotes are recorded here beside each kernel and not asserted: they are the
compiler's of the day.  The figures are the ones kmers_amd/build.py keeps per translation unit (-Rpass-analysis=kernel-resource-usage);
in a tree where the library has not been built the source is compiled here for gfx950.  Resource metadata only."""
from tests.kernel_usage import check_usage, usage_lines

# kernel -> (instances, VGPRs as DESIGN 4.6.22 quotes them, for the record; the most it may use; the most LDS)
STEMS = {"bgzf_inflate_kernel": (1, 93, 128, 40960), "bgzf_crc_kernel": (1, 16, 128, 40960), "bgzf_candidates_kernel": (2, 18, 128, 0),
         "bgzf_scan_kernel": (2, 70, 128, 1024), "bgzf_successor_kernel": (1, 14, 128, 0), "bgzf_mark_round_kernel": (1, 8, 128, 0),
         "bgzf_chain_stats_kernel": (1, 8, 128, 0), "bgzf_write_index_kernel": (1, 16, 128, 0)}


def test_bgzf_kernels_use_no_scratch(tmp_path):
    check_usage(STEMS, usage_lines("kmx_bgzf.hip", tmp_path))
