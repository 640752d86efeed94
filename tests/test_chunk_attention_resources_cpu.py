"""Resource guard for the chunk kernels (CPU: hipcc cross-compiles csrc/chunk_attention.hip for gfx950 and reads
-Rpass-analysis=kernel-resource-usage, the approach of tests/test_decode_resources_cpu.py): no scratch and no VGPR
spill in any instantiation, the occupancy the design states, and ``resource_table()`` is what
profiles/chunk_attention_resources.txt holds.  Reads resource figures only."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "distributed_lion_pytorch_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TABLE = ROOT / "profiles" / "chunk_attention_resources.txt"
# head_dim 128 with more than 32 query rows (T G > 32: 3 or 4 tiles) keeps Q^T in 16 and O^T in 32 registers per
# tile beside the K tile: more than the 256 two waves per SIMD leave, so these two run one block per CU (405 and
# 448 registers); every other kernel keeps two
ONE_BLOCK_PER_CU = {"chunk_attn_kernel<128, 3>", "chunk_attn_kernel<128, 4>"}


def chunk_resources(tmp_path):
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", f"-I{CSRC}", "--cuda-device-only", "-c",
           str(CSRC / "chunk_attention.hip"), "-o", str(Path(tmp_path) / "chunk_attention.o"),
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
    m = re.search(r"\d+(kv_append_chunk_kernel|chunk_attn_kernel|chunk_combine_kernel)ILi(\d+)E(?:Li(\d+)E)?", name)
    if not m:
        return name
    return f"{m.group(1)}<{m.group(2)}" + (f", {m.group(3)}>" if m.group(3) is not None else ">")


def _key(name: str):
    s = _short(name)
    return (s.split("<")[0], [int(x) for x in re.findall(r"\d+", s.split("<", 1)[1])] if "<" in s else [])


def resource_table(res) -> str:
    head = f"{'kernel':34s} {'VGPRs':>5s} {'AGPRs':>5s} {'SGPRs':>5s} {'LDS':>6s} {'scratch':>7s} {'VGPR spill':>10s} {'SGPR spill':>10s} {'waves/SIMD':>10s}"
    lines = ["# csrc/chunk_attention.hip for gfx950, -O3, -Rpass-analysis=kernel-resource-usage",
             "# kv_append_chunk_kernel<D, mode> (0 append, 1 rope, 2 norm + rope); chunk_attn_kernel<D, 16-row query tiles>;",
             "# chunk_combine_kernel<D>", head]
    for k in sorted(res, key=_key):
        v = res[k]
        lines.append(f"{_short(k):34s} {v['VGPRs']:5d} {v['AGPRs']:5d} {v['TotalSGPRs']:5d} {v['LDS Size [bytes/block]']:6d} "
                     f"{v['ScratchSize [bytes/lane]']:7d} {v['VGPRs Spill']:10d} {v['SGPRs Spill']:10d} "
                     f"{v['Occupancy [waves/SIMD]']:10d}")
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    return chunk_resources(tmp_path_factory.mktemp("chunk"))


def test_chunk_kernels_have_no_scratch_and_no_vgpr_spill(res):
    names = sorted(_short(k) for k in res)
    assert len([n for n in names if n.startswith("chunk_attn_kernel")]) == 8, names  # D in {64, 128} x 1..4 query tiles
    assert len([n for n in names if n.startswith("kv_append_chunk_kernel")]) == 6, names  # D x {append, rope, norm + rope}
    assert len([n for n in names if n.startswith("chunk_combine_kernel")]) == 2, names
    bad = {_short(k): v for k, v in res.items() if v["ScratchSize [bytes/lane]"] or v["VGPRs Spill"]}
    assert not bad, bad
    for k, v in res.items():
        # 256 threads are one wave per SIMD: two blocks per CU need two waves per SIMD (and 2 x LDS <= 160 KiB)
        need = 1 if _short(k) in ONE_BLOCK_PER_CU else 2
        assert v["Occupancy [waves/SIMD]"] >= need, (_short(k), v)
        assert 2 * v["LDS Size [bytes/block]"] <= 160 * 1024, (_short(k), v)


def test_recorded_table_is_current(res):
    assert TABLE.read_text() == resource_table(res), "regenerate profiles/chunk_attention_resources.txt (resource_table)"


if __name__ == "__main__":  # regenerate the recorded table
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        TABLE.parent.mkdir(parents=True, exist_ok=True)
        TABLE.write_text(resource_table(chunk_resources(d)))
