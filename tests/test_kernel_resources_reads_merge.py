"""What hipcc reports for the kernels of kmx_reads_merge.hip: no scratch at all, no dynamic stack and no spilled register, vector or
scalar.  The merge kernel -- four instances: with and without quality bytes, with and without the batch written -- stays within 64
VGPRs and uses no LDS; the two plan kernels use what their block scan and block sum take (2 048 and 32 bytes).  The
counts DESIGN quotes (63 VGPRs with quality bytes and outputs, 35 to 42 for the others; 22 and 32 for the plan) are recorded here
and not asserted: they are the compiler's of the day.  The figures are the ones kmers_amd/build.py keeps per translation unit
(-Rpass-analysis=kernel-resource-usage); in a tree where the library has not been built the source is compiled here for gfx950.
Resource metadata only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmers_amd", "csrc")
USAGE = os.path.join(CSRC, "_obj", "kmx_reads_merge.usage.txt")
# kernel -> (instances, VGPRs as DESIGN 4.6.17 quotes them, for the record; the most it may use; the most LDS)
STEMS = {"reads_merge_kernel": (4, "63 / 41 / 42 / 35", 64, 0), "reads_merge_plan_count_kernel": (1, "22", 64, 32),
         "reads_merge_plan_write_kernel": (1, "32", 64, 2048)}


def _usage_lines(tmp_path):
    if os.path.exists(USAGE):
        return open(USAGE).read().splitlines()
    from kmers_amd import build

    hipcc = build.hipcc()
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("no hipcc and no usage file next to the objects")
    r = subprocess.run([hipcc, *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kmx_reads_merge.hip"),
                        "-o", str(tmp_path / "kmx_reads_merge.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return build._split_usage(r.stderr)[0].splitlines()


def test_reads_merge_kernels_use_no_scratch(tmp_path):
    seen = {stem: 0 for stem in STEMS}
    for ln in _usage_lines(tmp_path):
        parts = [p.strip() for p in ln.strip().split("|")]
        if len(parts) < 2:
            continue
        stem = next((s for s in STEMS if s in parts[0]), None)
        if stem is None:
            continue
        d = {}
        for p in parts[1:]:
            key, _, v = p.rpartition(":")
            d[key.strip()] = v.strip()
        assert d["ScratchSize [bytes/lane]"] == "0", (parts[0], d)
        assert d["Dynamic Stack"] == "False", parts[0]
        assert d["VGPRs Spill"] == "0" and d["SGPRs Spill"] == "0", parts[0]
        assert int(d["VGPRs"]) <= STEMS[stem][2], (parts[0], d["VGPRs"])
        assert int(d["LDS Size [bytes/block]"]) <= STEMS[stem][3], (parts[0], d["LDS Size [bytes/block]"])
        seen[stem] += 1
    assert seen == {stem: v[0] for stem, v in STEMS.items()}, seen
