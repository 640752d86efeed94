"""CPU side of the any-width add+norm kernels: the width rule, the host mirror
of the dropout hash at a runtime width, and a register-spill guard over every
add_norm_* kernel (hipcc cross-compiles; approach of test_kernel_resources_cpu)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from distributed_lion_pytorch_amd._build import EXTRA_FLAGS
from distributed_lion_pytorch_amd.ops import fused

CSRC = Path(__file__).resolve().parent.parent / "distributed_lion_pytorch_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_norm_supported_rule():
    assert all(fused.norm_supported(C) for C in range(256, 8193, 8))
    assert all(fused.norm_supported(C) for C in fused.NORM_WIDTHS)
    assert fused.norm_supported(7168)
    for C in (64, 128, 248, 260, 8200, 1028):
        assert not fused.norm_supported(C), C


def test_norm_parts_follow_the_dispatch():
    # one wave per row up to 1024 (4 rows per block iteration), one block per row above
    assert fused._norm_parts(16384, 896) == fused._norm_parts(16384, 1024) == fused._NORM_PARTS_CAP
    assert fused._norm_parts(320, 1016) == 320 // 16
    assert fused._norm_parts(320, 1032) == 320 // 4
    assert fused._norm_parts(1, 896) == fused._norm_parts(1, 3584) == 1


def test_keep_mask_shape_and_flat_indexing():
    keep = fused.norm_dropout_keep(3, 896, 0.1, 7)
    assert keep.shape == (3, 896) and keep.dtype == torch.bool
    flat = fused.norm_dropout_keep(1, 3 * 896, 0.1, 7)
    assert torch.equal(keep.reshape(-1), flat.reshape(-1)[:3 * 896])
    assert 0.85 < keep.float().mean().item() < 0.95


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
def test_add_norm_kernels_do_not_spill(tmp_path):
    src = "norm_kernels.hip"
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", f"-I{CSRC}", *EXTRA_FLAGS.get(src, []), "-c",
           str(CSRC / src), "-o", str(tmp_path / (src + ".o")), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark: *(VGPRs Spill|SGPRs Spill): (\d+)", line)
        if m and name:
            res[name][m.group(1)] = int(m.group(2))
    kernels = {k: v for k, v in res.items() if "add_norm_" in k}
    # 10 exact + 10 tail shapes, LN / RMS, forward / backward
    assert sum("tail_kernel" in k for k in kernels) == 40 and len(kernels) == 80, sorted(kernels)
    assert all(set(v) == {"VGPRs Spill", "SGPRs Spill"} for v in kernels.values())
    spilled = {k: v for k, v in kernels.items() if v["VGPRs Spill"] or v["SGPRs Spill"]}
    assert not spilled, spilled
