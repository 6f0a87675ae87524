"""The headline instantiation scan_bitsliced_kernel<31, 10, 4> (k = 31 on 150-base ASCII reads), compiled to assembly here as
tests/test_kernel_resources.py does (device only, ~1 minute): its registers, and the shape of the two places whose LDS waits the code
is written around -- pass 2 of phase D as ONE basic block, and the byte-merge stages of the transpose waiting group by group."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "scan_bitsliced_kernelILi31ELi10ELi4ELb0ELb0ELb0EEEv"


@pytest.fixture(scope="module")
def headline(tmp_path_factory):
    """(resource remarks of the kernel, its assembly lines)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    sys.path.insert(0, ROOT)
    from kmers_amd import build as kb

    out = str(tmp_path_factory.mktemp("asm") / "kmx_bitslice.s")
    r = subprocess.run([hipcc, *kb.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                        os.path.join(kb.CSRC, "kmx_bitslice.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage = {}
    for ln in kb._split_usage(r.stderr)[0].splitlines():
        parts = [p.strip() for p in ln.split("|")]
        if HEADLINE in parts[0]:
            for p in parts[1:]:
                key, _, v = p.rpartition(":")
                usage[key.strip()] = v.strip()
    assert usage, "the headline instantiation is not in kmx_bitslice.hip"
    lines, body, inside = open(out).read().splitlines(), [], False
    for ln in lines:
        if re.match(r"^_Z\w+:", ln):
            inside = HEADLINE in ln
        if inside:
            body.append(ln)
            if "s_endpgm" in ln:
                break
    return usage, body


def test_headline_kernel_registers(headline):
    """three waves per SIMD hold at most 168 registers each; nothing in scratch"""
    usage, _ = headline
    assert int(usage["VGPRs"]) <= 168, usage
    assert int(usage["ScratchSize [bytes/lane]"]) == 0, usage
    assert usage["VGPRs Spill"] == "0" and usage["Dynamic Stack"] == "False", usage
    assert int(usage["Occupancy [waves/SIMD]"]) == 3, usage


def test_headline_pass2_is_one_basic_block(headline):
    """the 16 matrix products of a tile with no label and no branch between them, and every LDS request of the block ahead of the
    first product"""
    _, body = headline
    at = [i for i, ln in enumerate(body) if "v_mfma_scale_f32_32x32x64_f8f6f4" in ln]
    assert len(at) == 16, len(at)
    block = body[at[0]:at[-1] + 1]
    assert not [ln for ln in block if re.match(r"^\.LBB\d+_\d+:", ln) or "s_cbranch" in ln]
    assert not [ln for ln in block if re.match(r"\s*ds_read", ln)]


def test_headline_byte_merges_wait_group_by_group(headline):
    """stages xor-16 and xor-8: ten exchanges, then merge g behind s_waitcnt lgkmcnt(9 - g)"""
    _, body = headline
    for d in (16, 8):
        at = [i for i, ln in enumerate(body) if f"swizzle(SWAP,{d})" in ln]
        assert len(at) == 10, (d, len(at))
        run = [ln.strip() for ln in body[at[-1] + 1:at[-1] + 40] if re.match(r"\s*(s_waitcnt|v_perm_b32)", ln)][:20]
        assert [ln.split()[0] for ln in run] == ["s_waitcnt", "v_perm_b32"] * 10, (d, run)
        assert [re.search(r"lgkmcnt\((\d+)\)", ln).group(1) for ln in run[0::2]] == [str(9 - g) for g in range(10)], (d, run)
