"""Resource guard for the generation kernels (CPU: hipcc cross-compiles csrc/decode.hip for gfx950 and reads
-Rpass-analysis=kernel-resource-usage, the approach of tests/test_lm_score_resources_cpu.py): no scratch and no
VGPR spill in any instantiation, and ``resource_table()`` is what profiles/r12/decode_resources.txt holds."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributed_lion_pytorch_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TABLE = ROOT / "profiles" / "r12" / "decode_resources.txt"


def decode_resources(tmp_path):
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", f"-I{CSRC}", "--cuda-device-only", "-c",
           str(CSRC / "decode.hip"), "-o", str(Path(tmp_path) / "decode.o"), "-Rpass-analysis=kernel-resource-usage"]
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
    m = re.search(r"\d+(kv_append_kernel|decode_attn_kernel|decode_combine_kernel)ILi(\d+)E(?:Li(\d+)E)?", name)
    if not m:
        return name
    return f"{m.group(1)}<{m.group(2)}" + (f", {m.group(3)}>" if m.group(3) is not None else ">")


def _key(name: str):
    s = _short(name)
    return (s.split("<")[0], [int(x) for x in re.findall(r"\d+", s.split("<", 1)[1])] if "<" in s else [])


def resource_table(res) -> str:
    head = f"{'kernel':30s} {'VGPRs':>5s} {'AGPRs':>5s} {'SGPRs':>5s} {'LDS':>6s} {'scratch':>7s} {'VGPR spill':>10s} {'SGPR spill':>10s} {'waves/SIMD':>10s}"
    lines = ["# csrc/decode.hip for gfx950, -O3, -Rpass-analysis=kernel-resource-usage",
             "# kv_append_kernel<D, mode> (0 append, 1 rope, 2 norm + rope); decode_attn_kernel<D, group size rounded up>;",
             "# decode_combine_kernel<D>", head]
    for k in sorted(res, key=_key):
        v = res[k]
        lines.append(f"{_short(k):30s} {v['VGPRs']:5d} {v['AGPRs']:5d} {v['TotalSGPRs']:5d} {v['LDS Size [bytes/block]']:6d} "
                     f"{v['ScratchSize [bytes/lane]']:7d} {v['VGPRs Spill']:10d} {v['SGPRs Spill']:10d} "
                     f"{v['Occupancy [waves/SIMD]']:10d}")
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    return decode_resources(tmp_path_factory.mktemp("decode"))


def test_decode_kernels_have_no_scratch_and_no_vgpr_spill(res):
    names = sorted(_short(k) for k in res)
    assert len([n for n in names if n.startswith("decode_attn_kernel")]) == 8, names  # D in {64, 128} x group 1/2/4/8
    assert len([n for n in names if n.startswith("kv_append_kernel")]) == 6, names  # D x {append, rope, norm + rope}
    assert len([n for n in names if n.startswith("decode_combine_kernel")]) == 2, names
    bad = {_short(k): v for k, v in res.items() if v["ScratchSize [bytes/lane]"] or v["VGPRs Spill"]}
    assert not bad, bad
    for k, v in res.items():
        # 256 threads are one wave per SIMD: two blocks per CU need two waves per SIMD at the widest group
        assert v["Occupancy [waves/SIMD]"] >= 2, (_short(k), v)
        assert v["AGPRs"] == 0, (_short(k), v)


def test_recorded_table_is_current(res):
    assert TABLE.read_text() == resource_table(res), "regenerate profiles/r12/decode_resources.txt (resource_table)"


if __name__ == "__main__":  # regenerate the recorded table
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        TABLE.parent.mkdir(parents=True, exist_ok=True)
        TABLE.write_text(resource_table(decode_resources(d)))
