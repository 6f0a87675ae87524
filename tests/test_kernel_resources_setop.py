"""What hipcc reported for the kernels of kmx_count_setop.hip when libkmx was built (kmers_amd/build.py keeps
-Rpass-analysis=kernel-resource-usage per translation unit): no scratch at all and no dynamic stack, for either key width."""
import glob
import os
import re

import pytest

OBJ = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kmers_amd", "csrc", "_obj")


def _kernels():
    out = {}
    for f in glob.glob(os.path.join(OBJ, "*.usage.txt")):
        for ln in open(f):
            parts = [p.strip() for p in ln.strip().split("|")]
            if len(parts) < 2:
                continue
            d = {}
            for p in parts[1:]:
                k, _, v = p.rpartition(":")
                d[k.strip()] = v.strip()
            out[parts[0]] = d
    return out


def test_setop_kernels_use_no_scratch():
    kernels = _kernels()
    if not kernels:
        pytest.skip("no *.usage.txt next to the objects (library not built by kmers_amd.build in this tree)")
    seen = {1: 0, 2: 0}
    for name, d in kernels.items():
        if "setop" not in name:
            continue
        assert d["ScratchSize [bytes/lane]"] == "0", (name, d["ScratchSize [bytes/lane]"])
        assert d["Dynamic Stack"] == "False", name
        m = re.search(r"kernelILj([12])E", name)   # the first template argument: the words of a key
        assert m, name
        seen[int(m.group(1))] += 1
    # per key width: the partition, five count passes, five write passes, the comparison
    assert seen[1] >= 12 and seen[2] >= 12, seen
