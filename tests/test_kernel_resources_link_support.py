"""What hipcc reports for the kernels of kmx_count_link_support.hip: no scratch at all, no dynamic stack and no spilled register
(the kernels read indices, not keys: one instance each for both key widths), no LDS, and no more than 64 VGPRs -- what eight waves
per SIMD, the occupancy DESIGN 4.6.13 states, leave a wave.  The counts DESIGN quotes are recorded here beside each kernel and not
asserted: they are the compiler's of the day.  The figures are the ones kmers_amd/build.py keeps per translation unit
(-Rpass-analysis=kernel-resource-usage); in a tree where the library has not been built the source is compiled here for gfx950.
Resource metadata only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmers_amd", "csrc")
USAGE = os.path.join(CSRC, "_obj", "kmx_count_link_support.usage.txt")
# kernel -> (instances, VGPRs as DESIGN 4.6.13 quotes them, for the record)
STEMS = {"link_support_kernel": (1, 28), "adjacency_cut_kernel": (1, 24)}
MAX_VGPRS = 64   # 512 per SIMD lane / 8 waves


def _usage_lines(tmp_path):
    if os.path.exists(USAGE):
        return open(USAGE).read().splitlines()
    from kmers_amd import build

    hipcc = build.hipcc()
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("no hipcc and no usage file next to the objects")
    r = subprocess.run([hipcc, *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kmx_count_link_support.hip"),
                        "-o", str(tmp_path / "kmx_count_link_support.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return build._split_usage(r.stderr)[0].splitlines()


def test_link_support_kernels_use_no_scratch(tmp_path):
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
        assert int(d["VGPRs"]) <= MAX_VGPRS, (parts[0], d["VGPRs"])
        assert d["LDS Size [bytes/block]"] == "0", parts[0]
        seen[stem] += 1
    assert seen == {stem: n for stem, (n, _) in STEMS.items()}, seen
