"""Resource guard for the skinny-M GEMM (CPU: hipcc cross-compiles csrc/skinny_gemm.hip for gfx950 and reads
-Rpass-analysis=kernel-resource-usage, the approach of tests/test_decode_resources_cpu.py): no scratch, no VGPR
spill and at least 2 waves per SIMD in every instantiation, and ``resource_table()`` is what
profiles/r13/skinny_gemm_resources.txt holds."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributed_lion_pytorch_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TABLE = ROOT / "profiles" / "r13" / "skinny_gemm_resources.txt"


def skinny_resources(tmp_path):
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", f"-I{CSRC}", "--cuda-device-only", "-c",
           str(CSRC / "skinny_gemm.hip"), "-o", str(Path(tmp_path) / "skinny_gemm.o"),
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
    m = re.search(r"\d+skinny_gemm_kernelINS\d+_\d+(Weight\w+?)ELb([01])EEE", name)
    if m:
        return f"skinny_gemm_kernel<{m.group(1)}, {'tall' if m.group(2) == '1' else 'wide'}>"
    return "skinny_combine_kernel" if "skinny_combine_kernel" in name else name


def resource_table(res) -> str:
    head = f"{'kernel':38s} {'VGPRs':>5s} {'AGPRs':>5s} {'SGPRs':>5s} {'LDS':>6s} {'scratch':>7s} {'VGPR spill':>10s} {'SGPR spill':>10s} {'waves/SIMD':>10s}"
    lines = ["# csrc/skinny_gemm.hip for gfx950, -O3, -Rpass-analysis=kernel-resource-usage",
             "# skinny_gemm_kernel<weight format, wide: 4 row tiles per block | tall: the waves split K over one tile>;",
             "# the MFMA accumulators are the AGPRs", head]
    for k in sorted(res, key=_short):
        v = res[k]
        lines.append(f"{_short(k):38s} {v['VGPRs']:5d} {v['AGPRs']:5d} {v['TotalSGPRs']:5d} {v['LDS Size [bytes/block]']:6d} "
                     f"{v['ScratchSize [bytes/lane]']:7d} {v['VGPRs Spill']:10d} {v['SGPRs Spill']:10d} "
                     f"{v['Occupancy [waves/SIMD]']:10d}")
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    return skinny_resources(tmp_path_factory.mktemp("skinny"))


def test_skinny_kernels_have_no_scratch_no_spill_and_two_waves_per_simd(res):
    names = sorted(_short(k) for k in res)
    assert names == ["skinny_combine_kernel", "skinny_gemm_kernel<Weight4bit, tall>", "skinny_gemm_kernel<Weight4bit, wide>",
                     "skinny_gemm_kernel<WeightBf16, tall>", "skinny_gemm_kernel<WeightBf16, wide>"], names
    bad = {_short(k): v for k, v in res.items() if v["ScratchSize [bytes/lane]"] or v["VGPRs Spill"] or v["SGPRs Spill"]}
    assert not bad, bad
    for k, v in res.items():
        assert v["Occupancy [waves/SIMD]"] >= 2, (_short(k), v)
        # a CU's 160 KiB of LDS holds four blocks of the wide form (16 waves) and two of the tall form, whose x
        # chunk is four times as long and which runs at 2 waves per SIMD
        assert v["LDS Size [bytes/block]"] <= (80 if "tall" in _short(k) else 40) * 1024, (_short(k), v)


def test_recorded_table_is_current(res):
    assert TABLE.read_text() == resource_table(res), "regenerate profiles/r13/skinny_gemm_resources.txt (resource_table)"


if __name__ == "__main__":  # regenerate the recorded table
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        TABLE.parent.mkdir(parents=True, exist_ok=True)
        TABLE.write_text(resource_table(skinny_resources(d)))
