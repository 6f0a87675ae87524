"""What hipcc reports for the kernels of kmx_reads_edit.hip: no scratch at all, no dynamic stack and no spilled register.  The copy
kernel and the plan's count kernels stay within 64 VGPRs -- what eight waves per SIMD, the occupancy DESIGN 4.6.14 states for the
copy, leave a wave -- and the copy within the 16.5 KiB of LDS its staged offsets and source starts take; the plan's write kernels (eight clips per
thread in registers) are held to 128 VGPRs, four waves per SIMD.  The counts DESIGN quotes are recorded here beside each kernel and
not asserted: they are the compiler's of the day.  The figures are the ones kmers_amd/build.py keeps per translation unit
(-Rpass-analysis=kernel-resource-usage); in a tree where the library has not been built the source is compiled here for gfx950.
Resource metadata only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmers_amd", "csrc")
USAGE = os.path.join(CSRC, "_obj", "kmx_reads_edit.usage.txt")
# kernel -> (instances: select and gather, VGPRs as DESIGN 4.6.14 quotes them, for the record; the most it may use; the most LDS)
STEMS = {"reads_copy_kernel": (1, 48, 64, 16896), "reads_plan_count_kernel": (2, 22, 64, 64), "reads_plan_write_kernel": (2, 72, 128, 2048)}


def _usage_lines(tmp_path):
    if os.path.exists(USAGE):
        return open(USAGE).read().splitlines()
    from kmers_amd import build

    hipcc = build.hipcc()
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("no hipcc and no usage file next to the objects")
    r = subprocess.run([hipcc, *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kmx_reads_edit.hip"),
                        "-o", str(tmp_path / "kmx_reads_edit.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return build._split_usage(r.stderr)[0].splitlines()


def test_reads_edit_kernels_use_no_scratch(tmp_path):
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
