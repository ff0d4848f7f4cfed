"""The registers of the bit-sliced selection (csrc/mask_bits.hip) as the compiler reports them for gfx950, with the Makefile's
flags: the kernel's speed rests on four waves per SIMD for lists of at most 100 entries (H = 25: at most 128 VGPRs) and three for
longer ones (H = 32: at most 145 VGPRs, what it has had since it was written), without scratch. Two things in the source hold the
compiler to that -- the opaque plane offset of the gathers and the lane taken from v_mbcnt behind the loop (the comments there,
profiles/select_rounds_ab.txt) -- and nothing else would notice a compiler that stops honouring them. No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "repet-python_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops",
         "-mllvm", "-pragma-unroll-threshold=131072", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"]


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="no hipcc")
def test_selection_kernels_keep_their_waves_per_simd(tmp_path):
    run = subprocess.run([HIPCC, *FLAGS, "mask_bits.hip", "-o", str(tmp_path / "mask_bits.s")], cwd=SRC, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    found, name = {}, None
    for line in run.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, _, value = m.group(1).strip().partition(":")
        if key == "Function Name":
            k = re.search(r"mask_sim_bits_kernelILi(\d+)ELi(\d+)E", value)
            name = (int(k.group(1)), int(k.group(2))) if k else None
            if name:
                found[name] = {}
        elif name:
            found[name][key.strip()] = value.strip()
    assert sorted(found) == [(h, p) for h in (25, 32) for p in range(11, 16)], sorted(found)
    for (h, planes), r in sorted(found.items()):
        vgprs, scratch = int(r["VGPRs"]) + int(r.get("AGPRs", 0)), int(r["ScratchSize [bytes/lane]"])
        print("mask_sim_bits_kernel<%d, %d>: %d VGPRs, scratch %d, %s waves per SIMD" % (h, planes, vgprs, scratch, r.get("Occupancy [waves/SIMD]")))
        assert scratch == 0, (h, planes, r)
        assert vgprs <= (128 if h == 25 else 145), (h, planes, r)
