"""What hipcc reports for the deflate kernels of kmx_bgzf.hip: no scratch, no dynamic stack, no vector register spilled,
and LDS within what DESIGN states -- 32 KiB for the one wave a workgroup of the coding kernel is (five workgroups per CU of 160 KiB),
none for the copy and the tail kernel.  Register counts are the compiler's of the day: recorded beside each kernel as DESIGN quotes
them, printed, not asserted (the coding kernel keeps part of its scalar state in lanes of a vector register -- "SGPRs Spill" --
which costs no memory access).  The figures are the ones kmers_amd/build.py keeps per translation unit; in a tree where the library
has not been built the source is compiled here for gfx950.  Resource metadata only."""
from tests.kernel_usage import usage_lines

# kernel -> (VGPRs as DESIGN 4.6.23 quotes them, for the record; the most LDS)
STEMS = {"bgzf_deflate_kernel": (134, 32768), "bgzf_deflate_copy_kernel": (48, 0), "bgzf_deflate_tail_kernel": (4, 0)}


def test_bgzf_deflate_kernels_use_no_scratch(tmp_path):
    seen = {s: 0 for s in STEMS}
    for ln in usage_lines("kmx_bgzf.hip", tmp_path):
        parts = [p.strip() for p in ln.strip().split("|")]
        stem = next((s for s in STEMS if s in parts[0]), None)
        if stem is None:
            continue
        d = {}
        for p in parts[1:]:
            key, _, v = p.rpartition(":")
            d[key.strip()] = v.strip()
        print(stem, "VGPRs", d["VGPRs"], "SGPRs spilled to lanes", d["SGPRs Spill"], "LDS", d["LDS Size [bytes/block]"])
        assert d["ScratchSize [bytes/lane]"] == "0", (parts[0], d)
        assert d["Dynamic Stack"] == "False" and d["VGPRs Spill"] == "0", (parts[0], d)
        assert int(d["LDS Size [bytes/block]"]) <= STEMS[stem][1], (parts[0], d)
        seen[stem] += 1
    assert seen == {s: 1 for s in STEMS}, seen
