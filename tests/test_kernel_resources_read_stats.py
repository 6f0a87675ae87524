"""What hipcc reported for the kernels of kmx_count_read_stats.hip when libkmx was built (kmers_amd/build.py keeps
-Rpass-analysis=kernel-resource-usage per translation unit): no scratch at all and no dynamic stack in any instantiation."""
import os

import pytest

USAGE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kmers_amd", "csrc", "_obj", "kmx_count_read_stats.usage.txt")


def _kernels():
    out = {}
    if not os.path.exists(USAGE):
        return out
    for ln in open(USAGE):
        parts = [p.strip() for p in ln.strip().split("|")]
        if len(parts) < 2:
            continue
        d = {}
        for p in parts[1:]:
            k, _, v = p.rpartition(":")
            d[k.strip()] = v.strip()
        out[parts[0]] = d
    return out


def test_read_stats_kernels_use_no_scratch():
    kernels = _kernels()
    if not kernels:
        pytest.skip("no kmx_count_read_stats.usage.txt next to the objects (library not built by kmers_amd.build in this tree)")
    seen = {"short": 0, "long": 0}
    for name, d in kernels.items():   # every kernel of the translation unit, the shared ones of kmx_count_common.h included
        assert d["ScratchSize [bytes/lane]"] == "0", (name, d["ScratchSize [bytes/lane]"])
        assert d["Dynamic Stack"] == "False", name
        for kind in seen:
            if f"read_stats_{kind}" in name:
                seen[kind] += 1
    # the short kernel for 1, 2 and 4 registers per lane, uniform and ragged; the long one per wave, per block and for ragged reads
    assert seen["short"] >= 6 and seen["long"] >= 3, seen
