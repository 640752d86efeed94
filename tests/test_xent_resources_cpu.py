"""Resource guard for the LM-head cross-entropy kernels (CPU: hipcc cross-compiles
csrc/xent_kernels.hip for gfx950 and reads -Rpass-analysis=kernel-resource-usage,
the approach of tests/test_kernel_resources_cpu.py).

The label-smoothing / z-loss kernels are kernels of their own so that the plain
ones do not change: their VGPR / SGPR / LDS figures must be the ones recorded
below, taken from the commit before the options were added.  The options
kernels must report no scratch and no VGPR spill.  ``resource_table()`` is what
profiles/r10/xent_options_resources.txt holds."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "distributed_lion_pytorch_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# mangled kernel name -> (VGPRs, SGPRs, LDS bytes per block) before the options kernels existed
PLAIN = {
    "_ZN5dlion26softmax_xent_stream_kernelILi0EEEvPNS_4ElemIXT_EE1SEPKllliPf": (43, 80, 136),
    "_ZN5dlion19softmax_xent_kernelILi0ELi1EEEvPNS_4ElemIXT_EE1SEPKlliPf": (44, 48, 68),
    "_ZN5dlion19softmax_xent_kernelILi0ELi2EEEvPNS_4ElemIXT_EE1SEPKlliPf": (50, 50, 68),
    "_ZN5dlion19softmax_xent_kernelILi0ELi4EEEvPNS_4ElemIXT_EE1SEPKlliPf": (72, 54, 68),
    "_ZN5dlion19softmax_xent_kernelILi0ELi7EEEvPNS_4ElemIXT_EE1SEPKlliPf": (110, 60, 68),
    "_ZN5dlion19softmax_xent_kernelILi0ELi8EEEvPNS_4ElemIXT_EE1SEPKlliPf": (124, 62, 68),
    "_ZN5dlion26softmax_xent_packed_kernelILi1ELi1024ELi4EEEvPtPKlliPf": (44, 40, 128),
    "_ZN5dlion26softmax_xent_packed_kernelILi1ELi1024ELi7EEEvPtPKlliPf": (62, 46, 128),
    "_ZN5dlion26softmax_xent_packed_kernelILi1ELi256ELi16EEEvPtPKlliPf": (112, 64, 32),
    "_ZN5dlion26softmax_xent_packed_kernelILi1ELi256ELi25EEEvPtPKlliPf": (166, 82, 32),
    "_ZN5dlion26softmax_xent_packed_kernelILi1ELi512ELi8EEEvPtPKlliPf": (64, 48, 64),
    "_ZN5dlion26softmax_xent_packed_kernelILi1ELi512ELi13EEEvPtPKlliPf": (94, 58, 64),
    "_ZN5dlion26softmax_xent_packed_kernelILi1ELi512ELi16EEEvPtPKlliPf": (112, 64, 64),
    "_ZN5dlion26softmax_xent_stream_kernelILi1EEEvPNS_4ElemIXT_EE1SEPKllliPf": (45, 82, 136),
    "_ZN5dlion19softmax_xent_kernelILi1ELi1EEEvPNS_4ElemIXT_EE1SEPKlliPf": (44, 48, 68),
    "_ZN5dlion19softmax_xent_kernelILi1ELi2EEEvPNS_4ElemIXT_EE1SEPKlliPf": (46, 50, 68),
    "_ZN5dlion19softmax_xent_kernelILi1ELi4EEEvPNS_4ElemIXT_EE1SEPKlliPf": (68, 54, 68),
    "_ZN5dlion19softmax_xent_kernelILi1ELi7EEEvPNS_4ElemIXT_EE1SEPKlliPf": (106, 60, 68),
    "_ZN5dlion19softmax_xent_kernelILi1ELi8EEEvPNS_4ElemIXT_EE1SEPKlliPf": (124, 62, 68),
    "_ZN5dlion26softmax_xent_packed_kernelILi2ELi1024ELi4EEEvPtPKlliPf": (46, 40, 128),
    "_ZN5dlion26softmax_xent_packed_kernelILi2ELi1024ELi7EEEvPtPKlliPf": (64, 46, 128),
    "_ZN5dlion26softmax_xent_packed_kernelILi2ELi256ELi16EEEvPtPKlliPf": (110, 64, 32),
    "_ZN5dlion26softmax_xent_packed_kernelILi2ELi256ELi25EEEvPtPKlliPf": (164, 82, 32),
    "_ZN5dlion26softmax_xent_packed_kernelILi2ELi512ELi8EEEvPtPKlliPf": (62, 48, 64),
    "_ZN5dlion26softmax_xent_packed_kernelILi2ELi512ELi13EEEvPtPKlliPf": (92, 58, 64),
    "_ZN5dlion26softmax_xent_packed_kernelILi2ELi512ELi16EEEvPtPKlliPf": (110, 64, 64),
    "_ZN5dlion26softmax_xent_stream_kernelILi2EEEvPNS_4ElemIXT_EE1SEPKllliPf": (36, 86, 136),
    "_ZN5dlion19softmax_xent_kernelILi2ELi1EEEvPNS_4ElemIXT_EE1SEPKlliPf": (40, 48, 68),
    "_ZN5dlion19softmax_xent_kernelILi2ELi2EEEvPNS_4ElemIXT_EE1SEPKlliPf": (50, 50, 68),
    "_ZN5dlion19softmax_xent_kernelILi2ELi4EEEvPNS_4ElemIXT_EE1SEPKlliPf": (74, 54, 68),
    "_ZN5dlion19softmax_xent_kernelILi2ELi7EEEvPNS_4ElemIXT_EE1SEPKlliPf": (113, 60, 68),
    "_ZN5dlion19softmax_xent_kernelILi2ELi8EEEvPNS_4ElemIXT_EE1SEPKlliPf": (128, 62, 68),
}


def xent_resources(tmp_path):
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", f"-I{CSRC}", "--cuda-device-only", "-c",
           str(CSRC / "xent_kernels.hip"), "-o", str(Path(tmp_path) / "xent_kernels.o"),
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
    m = re.match(r"_ZN5dlion\d+(softmax_xent\w*?_kernel)I(.*?)EEEv", name)
    args = ", ".join(re.findall(r"Li(\d+)E", "Li" + m.group(2) + "E")) if m else ""
    return f"{m.group(1)}<{args}>" if m else name


def resource_table(res) -> str:
    head = f"{'kernel':48s} {'VGPRs':>5s} {'SGPRs':>5s} {'LDS':>5s} {'scratch':>7s} {'VGPR spill':>10s} {'SGPR spill':>10s} {'waves/SIMD':>10s}"
    lines = ["# csrc/xent_kernels.hip for gfx950, -O3, -Rpass-analysis=kernel-resource-usage",
             "# template arguments: dtype (0 fp32, 1 bf16, 2 fp16), then vectors per thread, or threads and chunks", head]
    for k in sorted(res, key=_short):
        v = res[k]
        lines.append(f"{_short(k):48s} {v['VGPRs']:5d} {v['TotalSGPRs']:5d} {v['LDS Size [bytes/block]']:5d} "
                     f"{v['ScratchSize [bytes/lane]']:7d} {v['VGPRs Spill']:10d} {v['SGPRs Spill']:10d} "
                     f"{v['Occupancy [waves/SIMD]']:10d}")
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    return xent_resources(tmp_path_factory.mktemp("xent"))


def test_plain_kernels_keep_their_resources(res):
    got = {k: (v["VGPRs"], v["TotalSGPRs"], v["LDS Size [bytes/block]"]) for k, v in res.items() if k in PLAIN}
    assert set(got) == set(PLAIN), sorted(set(PLAIN) - set(got))
    changed = {_short(k): (PLAIN[k], got[k]) for k in PLAIN if got[k] != PLAIN[k]}
    assert not changed, f"(VGPRs, SGPRs, LDS) before -> now: {changed}"


def test_options_kernels_have_no_scratch_and_no_vgpr_spill(res):
    opts = {k: v for k, v in res.items() if "_opts_kernel" in k}
    # fp32-row at 1, 2, 4, 7 vectors per thread and streaming for three dtypes; seven packed forms for two
    assert len(opts) == 3 * 4 + 3 + 2 * 7, sorted(_short(k) for k in opts)
    bad = {_short(k): v for k, v in opts.items() if v["ScratchSize [bytes/lane]"] or v["VGPRs Spill"]}
    assert not bad, bad
    # the default kernel of the GPT-2 and Llama-2 vocabularies keeps two 1024-thread blocks per CU (<= 64 VGPRs)
    for k, v in opts.items():
        if re.search(r"packed_opts_kernelILi[12]ELi1024E", k):
            assert v["VGPRs"] <= 64, (_short(k), v["VGPRs"])


def test_recorded_table_is_current(res):
    f = Path(__file__).resolve().parent.parent / "profiles" / "r10" / "xent_options_resources.txt"
    assert f.read_text() == resource_table(res), "regenerate profiles/r10/xent_options_resources.txt (resource_table)"
