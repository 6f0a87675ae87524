"""What hipcc reports for the two kernels of kmx_reads_adapter.hip: no scratch at all, no dynamic stack and no spilled register,
vector or scalar (the adapter kernel indexes the adapters' plane words in its kernel arguments with a loop counter: an argument
struct copied to the stack would show here first).  Both stay within 64 VGPRs -- what eight waves per SIMD, the occupancy DESIGN
4.6.16 states, leave a wave; the adapter kernel uses no LDS, the pair kernel the 3 456 bytes of its plane words (four waves x two
mates x three planes x 18 words), within 4 KiB.  The counts DESIGN quotes (28 and 48 VGPRs) are recorded here and not asserted: they
are the compiler's of the day.  The figures are the ones kmers_amd/build.py keeps per translation unit
(-Rpass-analysis=kernel-resource-usage); in a tree where the library has not been built the source is compiled here for gfx950.
Resource metadata only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmers_amd", "csrc")
USAGE = os.path.join(CSRC, "_obj", "kmx_reads_adapter.usage.txt")
# kernel -> (instances, VGPRs as DESIGN 4.6.16 quotes them, for the record; the most it may use; the most LDS)
STEMS = {"reads_adapter_kernel": (1, 28, 64, 0), "reads_pair_overlap_kernel": (1, 48, 64, 4096)}


def _usage_lines(tmp_path):
    if os.path.exists(USAGE):
        return open(USAGE).read().splitlines()
    from kmers_amd import build

    hipcc = build.hipcc()
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("no hipcc and no usage file next to the objects")
    r = subprocess.run([hipcc, *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kmx_reads_adapter.hip"),
                        "-o", str(tmp_path / "kmx_reads_adapter.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return build._split_usage(r.stderr)[0].splitlines()


def test_reads_adapter_kernels_use_no_scratch(tmp_path):
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
