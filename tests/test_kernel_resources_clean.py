"""What hipcc reports for the kernel of kmx_count_clean.hip: no scratch at all, no dynamic stack, no spilled register, no LDS, and no
more than 64 VGPRs -- what eight waves per SIMD, the occupancy DESIGN 4.6.9 states, leave a wave.  The rule has a dozen ways out and
every divergent level costs a pair of scalar registers: written with early returns the kernel spilled 32 of them, which is why its
conditions are gathered into flags, and what this test would show first.  The VGPR count DESIGN quotes is recorded here and not
asserted: it is the compiler's of the day.  The figures are the ones kmers_amd/build.py keeps per translation unit
(-Rpass-analysis=kernel-resource-usage); in a tree where the library has not been built the source is compiled here for gfx950.
Resource metadata only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmers_amd", "csrc")
USAGE = os.path.join(CSRC, "_obj", "kmx_count_clean.usage.txt")
STEMS = {"unitig_clean_kernel": (1, 38)}   # kernel -> (instances, VGPRs as DESIGN 4.6.9 quotes them, for the record)
MAX_VGPRS = 64   # 512 per SIMD lane / 8 waves


def _usage_lines(tmp_path):
    if os.path.exists(USAGE):
        return open(USAGE).read().splitlines()
    from kmers_amd import build

    hipcc = build.hipcc()
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("no hipcc and no usage file next to the objects")
    r = subprocess.run([hipcc, *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kmx_count_clean.hip"), "-o",
                        str(tmp_path / "kmx_count_clean.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return build._split_usage(r.stderr)[0].splitlines()


def test_clean_kernel_uses_no_scratch_and_no_lds(tmp_path):
    seen = {stem: 0 for stem in STEMS}
    kernels = 0
    for ln in _usage_lines(tmp_path):
        parts = [p.strip() for p in ln.strip().split("|")]
        if len(parts) < 2:
            continue
        kernels += 1
        stem = next((s for s in STEMS if s in parts[0]), None)
        if stem is None:
            continue
        d = {}
        for p in parts[1:]:
            key, _, v = p.rpartition(":")
            d[key.strip()] = v.strip()
        assert d["ScratchSize [bytes/lane]"] == "0", (parts[0], d)
        assert d["Dynamic Stack"] == "False", parts[0]
        assert d["VGPRs Spill"] == "0" and d["SGPRs Spill"] == "0", (parts[0], d)
        assert d["LDS Size [bytes/block]"] == "0", parts[0]
        assert int(d["VGPRs"]) <= MAX_VGPRS, (parts[0], d["VGPRs"])
        seen[stem] += 1
    assert seen == {stem: n for stem, (n, _) in STEMS.items()}, seen
    assert kernels == 1                                                      # the translation unit holds this kernel and nothing else
