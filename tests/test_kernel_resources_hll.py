"""What hipcc reports for the kernels of kmx_hll.hip: no scratch at all, no dynamic stack and no spilled register, vector or scalar,
and every kernel within 64 VGPRs (eight waves per SIMD, the family's convention).  LDS is exactly what DESIGN 4.6.24 states: the
block-private instances of the add kernel hold the register array at the cut and nothing else (1 << 14 bytes), the global instances
none, the merge none, the stats kernel its 3 * 64 bins of four bytes.  The VGPR counts DESIGN quotes (11 for the add, 30 and 40 for
merge and stats) are recorded here and not asserted: they are the compiler's of the day.  The figures are the ones
kmers_amd/build.py keeps per translation unit (-Rpass-analysis=kernel-resource-usage); in a tree where the library has not been built
the source is compiled here for gfx950.  Resource metadata only."""
from kmers_amd import _lib
from tests.kernel_usage import check_usage, usage_lines

REGS_AT_THE_CUT = 1 << _lib.HLL_LDS_MAX_LOG2_REGS
STATS_BINS = 3 * _lib.HLL_BINS * 4
# kernel -> (instances, VGPRs as DESIGN 4.6.24 quotes them, for the record; the most it may use; its LDS, exactly)
STEMS = {"hll_add_kernelILj1ELb1E": (1, "11", 64, REGS_AT_THE_CUT), "hll_add_kernelILj2ELb1E": (1, "11", 64, REGS_AT_THE_CUT),
         "hll_add_kernelILj1ELb0E": (1, "11", 64, 0), "hll_add_kernelILj2ELb0E": (1, "11", 64, 0),
         "hll_merge_kernel": (1, "30", 64, 0), "hll_stats_kernel": (1, "40", 64, STATS_BINS)}


def test_hll_kernels_use_no_scratch_and_exactly_their_lds(tmp_path):
    lines = usage_lines("kmx_hll.hip", tmp_path)
    check_usage(STEMS, lines)
    assert REGS_AT_THE_CUT == 16384 and STATS_BINS == 768
    seen = 0
    for ln in lines:
        parts = [p.strip() for p in ln.strip().split("|")]
        stem = next((s for s in STEMS if s in parts[0]), None)
        if stem is None:
            continue
        lds = next(p for p in parts[1:] if p.startswith("LDS Size")).rpartition(":")[2].strip()
        assert int(lds) == STEMS[stem][3], (parts[0], lds)
        seen += 1
    assert seen == len(STEMS)
