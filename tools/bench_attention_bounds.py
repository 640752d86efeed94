"""Bounds (document-isolated) vs plain-causal flash attention kernels on the
same tensors in one process: B=4, T=1024, H=Hkv=32, D=128, three documents
per row (the Llama-2-7B SFT shape with stack-exchange-sized samples).

Run under the kernel timer, then read its per-dispatch trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o prof -- \\
        python tools/bench_attention_bounds.py [B T H Hkv]
    python tools/bench_attention_bounds.py --parse <dir>/.../prof_kernel_trace.csv

Rounds alternate REPS plain and REPS bounds forward + backward passes; the
parser prints, per kernel, the median of the per-round mean times and their
min .. max -- the spread of repeated runs that a difference has to exceed."""
import csv
import os
import statistics
import sys

ROUNDS, REPS = 6, 10


def run(argv):
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from distributed_lion_pytorch_amd.ops import fused, hip

    hip.require()
    B, T, H, Hkv = [int(x) for x in argv] if len(argv) == 4 else (4, 1024, 32, 32)
    D, dev = 128, "cuda"
    torch.manual_seed(0)
    q = torch.randn(B, T, H, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(B, T, Hkv, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(B, T, Hkv, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    dout = torch.randn(B, T, H, D, device=dev, dtype=torch.bfloat16)
    # three documents per row, a different split in every row
    cuts = [(300 + 37 * b, 700 - 53 * b) for b in range(B)]
    pos = torch.stack([torch.cat([torch.arange(a), torch.arange(c - a), torch.arange(T - c)]) for a, c in cuts]).to(dev)
    bounds = fused.visibility_bounds(pos)

    def step(bd):
        fused._FlashAttn.apply(q, k, v, 0.0, 0, 0, bd).backward(dout)

    step(None)  # one warm-up dispatch of each kernel: the parser drops it
    step(bounds)
    for _ in range(ROUNDS):
        for bd in (None, bounds):
            for _ in range(REPS):
                step(bd)
    torch.cuda.synchronize()
    print(f"B={B} T={T} H={H}/{Hkv} D={D} documents per row {[(a, c - a, T - c) for a, c in cuts]}")


def parse(path):
    per = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "attn_" not in name:
                continue
            short = name.split("(")[0].replace("void dlion::", "")
            per.setdefault(short, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    print(f"{'kernel':<46}{'median us':>10}{'min':>9}{'max':>9}   (per-round means, {ROUNDS} rounds x {REPS})")
    for short in sorted(per):
        d = [(e - s) / 1000.0 for s, e in sorted(per[short])][1:]  # without the warm-up dispatch
        rounds = [statistics.mean(d[i:i + REPS]) for i in range(0, len(d) - REPS + 1, REPS)]
        print(f"{short:<46}{statistics.median(rounds):>10.1f}{min(rounds):>9.1f}{max(rounds):>9.1f}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--parse":
        parse(sys.argv[2])
    else:
        run(sys.argv[1:])
