"""What hipcc reports for the kernels of kmx_count_correct.hip: no scratch at all, no dynamic stack, no spilled register -- vector or
scalar --, no LDS in the decision kernel, and no more than 96 VGPRs in it: what five waves per SIMD, the occupancy DESIGN 4.6.10
states, leave a wave.  Scalar registers are what this kernel runs out of first: every lane predicate of the lockstep searches is a
pair of them, on top of seventeen kernel arguments and the wave's loop state -- written with the table's arguments left in scalar
registers the two-word directory instance spilled 21, which is why the kernel moves what it only ever combines with per-lane values
into vector registers (in_vgpr), and what this test would show first.  The VGPR counts DESIGN quotes are recorded here and not
asserted: they are the compiler's of the day.  The two compaction kernels every user of kmx_count_common.h compiles come along in the
object (they are not launched from here); the scratch / stack / spill conditions are asked of them too.  The figures are the ones
kmers_amd/build.py keeps per translation unit (-Rpass-analysis=kernel-resource-usage); in a tree where the library has not been
built the source is compiled here for gfx950.  Resource metadata only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmers_amd", "csrc")
USAGE = os.path.join(CSRC, "_obj", "kmx_count_correct.usage.txt")
# kernel -> VGPRs as DESIGN 4.6.10 quotes them, for the record: <W, DIR> = <1, true>, <1, false>, <2, true>, <2, false>
STEMS = {"correct_kernelILj1ELb1E": 78, "correct_kernelILj1ELb0E": 74, "correct_kernelILj2ELb1E": 88, "correct_kernelILj2ELb0E": 86}
MAX_VGPRS = 96   # 512 per SIMD lane / 5 waves, in allocation blocks of 8
LDS_BYTES = 0    # the decision kernel keeps its history in ballots: no LDS


def _usage_lines(tmp_path):
    if os.path.exists(USAGE):
        return open(USAGE).read().splitlines()
    from kmers_amd import build

    hipcc = build.hipcc()
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("no hipcc and no usage file next to the objects")
    r = subprocess.run([hipcc, *build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kmx_count_correct.hip"), "-o",
                        str(tmp_path / "kmx_count_correct.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return build._split_usage(r.stderr)[0].splitlines()


def test_correct_kernels_use_no_scratch_no_lds_and_spill_nothing(tmp_path):
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
        assert d["LDS Size [bytes/block]"] == str(LDS_BYTES), parts[0]
        assert int(d["VGPRs"]) <= MAX_VGPRS, (parts[0], d["VGPRs"])
        seen[stem] += 1
    assert seen == {stem: 1 for stem in STEMS}, seen
    assert kernels == len(STEMS) + 2                                         # ... and the two compaction kernels of kmx_count_common.h
