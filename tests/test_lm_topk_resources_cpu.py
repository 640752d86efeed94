"""Resource guard for the LM-head top-k kernels (CPU: hipcc cross-compiles
csrc/lm_topk.hip for gfx950 and reads -Rpass-analysis=kernel-resource-usage,
the approach of tests/test_lm_score_resources_cpu.py): no scratch and no VGPR
spill in any instantiation, and ``resource_table()`` is what
profiles/r14/lm_topk_resources.txt holds."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributed_lion_pytorch_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TABLE = ROOT / "profiles" / "r14" / "lm_topk_resources.txt"


def topk_resources(tmp_path):
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", f"-I{CSRC}", "--cuda-device-only", "-c",
           str(CSRC / "lm_topk.hip"), "-o", str(Path(tmp_path) / "lm_topk.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark: +([A-Za-z \[\]/]+): (\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def _short(name: str) -> str:
    m = re.match(r"_ZN5dlion\d+(lm_topk\w*?_kernel)ILi(\d+)E", name)
    return f"{m.group(1)}<{m.group(2)}>" if m else name


def resource_table(res) -> str:
    head = f"{'kernel':24s} {'VGPRs':>5s} {'SGPRs':>5s} {'LDS':>5s} {'scratch':>7s} {'VGPR spill':>10s} {'SGPR spill':>10s} {'waves/SIMD':>10s}"
    lines = ["# csrc/lm_topk.hip for gfx950, -O3, -Rpass-analysis=kernel-resource-usage",
             "# template argument: dtype (0 fp32, 1 bf16, 2 fp16)", head]
    for k in sorted(res, key=_short):
        v = res[k]
        lines.append(f"{_short(k):24s} {v['VGPRs']:5d} {v['TotalSGPRs']:5d} {v['LDS Size [bytes/block]']:5d} "
                     f"{v['ScratchSize [bytes/lane]']:7d} {v['VGPRs Spill']:10d} {v['SGPRs Spill']:10d} "
                     f"{v['Occupancy [waves/SIMD]']:10d}")
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    return topk_resources(tmp_path_factory.mktemp("lm_topk"))


def test_topk_kernels_have_no_scratch_and_no_vgpr_spill(res):
    kernels = {k: v for k, v in res.items() if "lm_topk" in k}
    assert len(kernels) == 3, sorted(_short(k) for k in kernels)  # one per dtype
    bad = {_short(k): v for k, v in kernels.items() if v["ScratchSize [bytes/lane]"] or v["VGPRs Spill"]}
    assert not bad, bad


def test_recorded_table_is_current(res):
    assert TABLE.read_text() == resource_table(res), "regenerate profiles/r14/lm_topk_resources.txt (resource_table)"


if __name__ == "__main__":  # regenerate the recorded table
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        TABLE.parent.mkdir(parents=True, exist_ok=True)
        TABLE.write_text(resource_table(topk_resources(d)))
