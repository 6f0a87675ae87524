"""What the test_kernel_resources_reads_*.py files share: the resource lines hipcc reports for the kernels of one translation unit, and
the check of them against a table of kernel stems.  The figures are the ones kmers_amd/build.py keeps per translation unit
(-Rpass-analysis=kernel-resource-usage); in a tree where the library has not been built the source is compiled here for gfx950.
Resource metadata only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmers_amd", "csrc")


def usage_lines(source_name, tmp_path):
    """one line per kernel of kmers_amd/csrc/<source_name>: its name and resources"""
    stem = os.path.splitext(source_name)[0]
    usage = os.path.join(CSRC, "_obj", stem + ".usage.txt")
    if os.path.exists(usage):
        return open(usage).read().splitlines()
    from kmers_amd import build

    hipcc = build.hipcc()
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("no hipcc and no usage file next to the objects")
    r = subprocess.run([hipcc, *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, source_name),
                        "-o", str(tmp_path / (stem + ".o"))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return build._split_usage(r.stderr)[0].splitlines()


def check_usage(stems, lines):
    """stems: kernel stem -> (instances, VGPRs as DESIGN quotes them, for the record; the most it may use; the most LDS).  Every kernel
    whose name holds a stem: no scratch, no dynamic stack, no spill, within its VGPR and LDS bounds; and as many instances as stated."""
    seen = {stem: 0 for stem in stems}
    for ln in lines:
        parts = [p.strip() for p in ln.strip().split("|")]
        if len(parts) < 2:
            continue
        stem = next((s for s in stems if s in parts[0]), None)
        if stem is None:
            continue
        d = {}
        for p in parts[1:]:
            key, _, v = p.rpartition(":")
            d[key.strip()] = v.strip()
        assert d["ScratchSize [bytes/lane]"] == "0", (parts[0], d)
        assert d["Dynamic Stack"] == "False", parts[0]
        assert d["VGPRs Spill"] == "0" and d["SGPRs Spill"] == "0", parts[0]
        assert int(d["VGPRs"]) <= stems[stem][2], (parts[0], d["VGPRs"])
        assert int(d["LDS Size [bytes/block]"]) <= stems[stem][3], (parts[0], d["LDS Size [bytes/block]"])
        seen[stem] += 1
    assert seen == {stem: v[0] for stem, v in stems.items()}, seen
