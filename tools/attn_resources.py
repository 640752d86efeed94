"""Resource table of the attention kernels (VGPRs, AGPRs, SGPRs, scratch, LDS,
occupancy, spills), from hipcc's -Rpass-analysis=kernel-resource-usage with
the build's flags -- the spill guard's compile (tests/test_kernel_resources_cpu.py).

    python tools/attn_resources.py [csrc dir]  > table

Kernels are listed by demangled name.  A trailing defaulted ``false`` template
argument is dropped from the name (``--raw`` keeps it), so a table taken before
a defaulted parameter was added lines up row by row with one taken after."""
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from distributed_lion_pytorch_amd._build import EXTRA_FLAGS  # noqa: E402

FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
          "Occupancy [waves/SIMD]", "VGPRs Spill", "SGPRs Spill"]


def resources(csrc: Path) -> dict:
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", f"-I{csrc}", *EXTRA_FLAGS.get("attention.hip", []),
               "-c", str(csrc / "attention.hip"), "-o", str(Path(tmp) / "attention.o"),
               "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr[-4000:])
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark: *([A-Za-z][^:]*): (\d+)", line)
        if m and name and m.group(1).strip() in FIELDS:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def demangle(names):
    """attn_x_kernel<int / bool template arguments> from the Itanium name."""
    out = []
    for n in names:
        m = re.search(r"\d+(attn_\w+_kernel)I((?:L[ib]\d+E)+)E", n)
        if not m:
            out.append(n)
            continue
        args = [v if k == "i" else ("true" if v == "1" else "false") for k, v in re.findall(r"L([ib])(\d+)E", m.group(2))]
        out.append(f"{m.group(1)}<{', '.join(args)}>")
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--raw"]
    raw = "--raw" in sys.argv[1:]
    csrc = Path(args[0]) if args else ROOT / "distributed_lion_pytorch_amd" / "csrc"
    res = {k: v for k, v in resources(csrc).items() if "attn_" in k}
    rows = []
    for mangled, nice in zip(res, demangle(list(res))):
        nice = re.sub(r"^void dlion::|\(dlion::AttnArgs\)$", "", nice)
        if not raw:
            nice = re.sub(r"(, false)>$", ">", nice) if nice.count(",") == 3 else nice
        rows.append((nice, res[mangled]))
    print(f"{'kernel':<48}" + "".join(f"{h:>9}" for h in ["VGPR", "AGPR", "SGPR", "scratch", "LDS", "occ", "vspill", "sspill"]))
    for nice, v in sorted(rows):
        print(f"{nice:<48}" + "".join(f"{v.get(f, 0):>9}" for f in FIELDS))


if __name__ == "__main__":
    main()
