"""What hipcc reported for the kernels of kmx_count_graph.hip when libkmx was built (kmers_amd/build.py keeps
-Rpass-analysis=kernel-resource-usage per translation unit): no scratch at all and no dynamic stack, for either key width."""
import glob
import os
import re

import pytest

OBJ = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kmers_amd", "csrc", "_obj")
STEMS = ("adjacency_kernel", "edge_hist_kernel", "unitig_ends_kernel")


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


def test_graph_kernels_use_no_scratch():
    kernels = _kernels()
    if not kernels:
        pytest.skip("no *.usage.txt next to the objects (library not built by kmers_amd.build in this tree)")
    seen = {stem: 0 for stem in STEMS}
    widths = {1: 0, 2: 0}
    for name, d in kernels.items():
        stem = next((s for s in STEMS if s in name), None)
        if stem is None:
            continue
        assert d["ScratchSize [bytes/lane]"] == "0", (name, d["ScratchSize [bytes/lane]"])
        assert d["Dynamic Stack"] == "False", name
        assert d["VGPRs Spill"] == "0", name
        seen[stem] += 1
        m = re.search(r"adjacency_kernelILj([12])E", name)   # the first template argument: the words of a key
        if m:
            widths[int(m.group(1))] += 1
    # per key width: with and without the directory, with and without flips / indices; one histogram, one ends kernel
    assert widths == {1: 4, 2: 4}, widths
    assert seen["edge_hist_kernel"] == 1 and seen["unitig_ends_kernel"] == 1, seen
