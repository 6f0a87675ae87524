"""What hipcc reports for the kernels of kmx_count_color.hip: no scratch at all, no dynamic stack, no spilled register -- vector or
scalar.  The per-read kernel uses no LDS and no more than 64 VGPRs: what eight waves per SIMD, the occupancy DESIGN 4.6.11 states,
leave a wave.  The matrix kernels fold their four waves in LDS: CB * 64 u32 for the tile and 65 u32 for the spectrum, CB = 8 / 16 /
32 / 64 -- the sizes DESIGN states, asserted here.  Scalar registers are what the 64-colour matrix kernel would run out of first: its
transpose written as a select on `lane == i` had 64 loop-invariant lane predicates hoisted into scalar register pairs and spilled 62
(v_writelane with the lane as an immediate keeps none), which is what this test would show first.  The VGPR counts DESIGN quotes
are recorded here and not asserted: they are the compiler's of the day.  The two kernels every user of kmx_count_common.h compiles
come along in the object (they are not launched from here); the scratch / stack / spill conditions are asked of them too.  The
figures are the ones kmers_amd/build.py keeps per translation unit (-Rpass-analysis=kernel-resource-usage); in a tree where the
library has not been built the source is compiled here for gfx950.  Resource metadata only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmers_amd", "csrc")
USAGE = os.path.join(CSRC, "_obj", "kmx_count_color.usage.txt")
# kernel -> (VGPRs as DESIGN 4.6.11 quotes them, for the record; LDS bytes, asserted)
STEMS = {"read_colors_kernel": (22, 0), "color_sum_kernel": (14, 2048),
         "color_matrix_kernelILj8E": (21, 4 * (8 * 64 + 65)), "color_matrix_kernelILj16E": (29, 4 * (16 * 64 + 65)),
         "color_matrix_kernelILj32E": (44, 4 * (32 * 64 + 65)), "color_matrix_kernelILj64E": (79, 4 * (64 * 64 + 65))}
READ_MAX_VGPRS = 64   # 512 per SIMD lane / 8 waves


def _usage_lines(tmp_path):
    if os.path.exists(USAGE):
        return open(USAGE).read().splitlines()
    from kmers_amd import build

    hipcc = build.hipcc()
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("no hipcc and no usage file next to the objects")
    r = subprocess.run([hipcc, *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kmx_count_color.hip"), "-o",
                        str(tmp_path / "kmx_count_color.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return build._split_usage(r.stderr)[0].splitlines()


def test_color_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    seen = {stem: 0 for stem in STEMS}
    kernels = 0
    for ln in _usage_lines(tmp_path):
        parts = [p.strip() for p in ln.strip().split("|")]
        if len(parts) < 2:
            continue
        kernels += 1
        d = {}
        for p in parts[1:]:
            key, _, v = p.rpartition(":")
            d[key.strip()] = v.strip()
        assert d["ScratchSize [bytes/lane]"] == "0", (parts[0], d)
        assert d["Dynamic Stack"] == "False", parts[0]
        assert d["VGPRs Spill"] == "0" and d["SGPRs Spill"] == "0", (parts[0], d)
        stem = next((s for s in STEMS if s in parts[0]), None)
        if stem is None:
            continue
        assert d["LDS Size [bytes/block]"] == str(STEMS[stem][1]), (parts[0], d)
        if stem == "read_colors_kernel":
            assert int(d["VGPRs"]) <= READ_MAX_VGPRS, (parts[0], d["VGPRs"])
            assert d["Occupancy [waves/SIMD]"] == "8", (parts[0], d)
        seen[stem] += 1
    assert seen == {stem: 1 for stem in STEMS}, seen
    assert kernels == len(STEMS) + 2                                         # ... and the two kernels of kmx_count_common.h
