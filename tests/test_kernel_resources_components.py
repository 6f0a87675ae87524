"""What hipcc reports for the kernels of kmx_count_components.hip: no scratch, no dynamic stack, no spilled register, no more than 64
VGPRs -- what eight waves per SIMD, the occupancy DESIGN 4.6.12 states, leave a wave: the hook, jump and gather kernels are
latency-bound gathers, and lanes in flight are what hides them -- and LDS only in the kernels that scan (the ranges' root counts, the
scan over them, the ranks; and the compaction's count kernel that the family's header brings along, which this call never
launches).  The hook kernel has a validity condition per list, per target and per mask byte; as in kmx_count_clean.hip they are
gathered into flags instead of early exits, and a spilled scalar register is what this test would show first.  The VGPR counts
DESIGN quotes are recorded here and not asserted: they are the compiler's of the day.  The figures are the ones kmers_amd/build.py
keeps per translation unit (-Rpass-analysis=kernel-resource-usage); in a tree where the library has not been built the source is
compiled here for gfx950.  Resource metadata only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmers_amd", "csrc")
SRC = "kmx_count_components.hip"
USAGE = os.path.join(CSRC, "_obj", "kmx_count_components.usage.txt")
# kernel -> (it scans: LDS allowed, VGPRs as DESIGN 4.6.12 quotes them, for the record)
STEMS = {"component_init_kernel": (False, 6), "component_hook_kernel": (False, 22), "component_jump_kernel": (False, 12),
         "component_roots_kernel": (True, 11), "component_rank_kernel": (True, 46), "component_gather_kernel": (False, 32),
         "scan_single_kernel": (True, 38), "keep_count_kernel": (True, 22)}
MAX_VGPRS = 64   # 512 per SIMD lane / 8 waves


def _usage_lines(tmp_path):
    if os.path.exists(USAGE):
        return open(USAGE).read().splitlines()
    from kmers_amd import build

    hipcc = build.hipcc()
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("no hipcc and no usage file next to the objects")
    r = subprocess.run([hipcc, *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, SRC), "-o",
                        str(tmp_path / "kmx_count_components.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return build._split_usage(r.stderr)[0].splitlines()


def test_component_kernels_use_no_scratch_and_lds_only_to_scan(tmp_path):
    seen = {stem: 0 for stem in STEMS}
    for ln in _usage_lines(tmp_path):
        parts = [p.strip() for p in ln.strip().split("|")]
        if len(parts) < 2:
            continue
        stem = next((s for s in STEMS if s in parts[0]), None)
        assert stem is not None, parts[0]                                    # every kernel of the translation unit is one of these
        d = {}
        for p in parts[1:]:
            key, _, v = p.rpartition(":")
            d[key.strip()] = v.strip()
        assert d["ScratchSize [bytes/lane]"] == "0", (parts[0], d)
        assert d["Dynamic Stack"] == "False", parts[0]
        assert d["VGPRs Spill"] == "0" and d["SGPRs Spill"] == "0", (parts[0], d)
        assert STEMS[stem][0] or d["LDS Size [bytes/block]"] == "0", (parts[0], d["LDS Size [bytes/block]"])
        assert int(d["VGPRs"]) <= MAX_VGPRS, (parts[0], d["VGPRs"])
        seen[stem] += 1
    assert seen == {stem: 1 for stem in STEMS}, seen


def test_source_is_part_of_the_build():
    from kmers_amd import build

    assert SRC in build.SOURCES and os.path.join(CSRC, "kmx_count_common.h") in build._headers_of(SRC)
