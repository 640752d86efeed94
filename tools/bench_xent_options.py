"""Plain against options form of the fused softmax-xent kernel (label smoothing /
z-loss), on the same tensors in one process, alternating call by call.

    python tools/bench_xent_options.py [--smoothing 0.1] [--z_loss 1e-3] [--reps 40] [--out FILE]

Shapes: the GPT-2 bench rows (20460 x 50304), Llama-2 (8192 x 32000) and
Llama-3 (8192 x 128256), bf16.  Per form: the median device time, the p10-p90
spread and the row traffic rate (one read and one write of the row; the
streaming kernel's second read is not counted)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_lion_pytorch_amd.ops import hip  # noqa: E402

SHAPES = [(20460, 50304), (8192, 32000), (8192, 128256)]


def _q(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--smoothing", type=float, default=0.1)
    ap.add_argument("--z_loss", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--variant", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    hip.require()
    ops = hip.ops()
    lines = [f"# plain vs options (smoothing {a.smoothing}, z_loss {a.z_loss}), variant {a.variant}, "
             f"{a.reps} alternating reps, bf16, {torch.cuda.get_device_name(0)}"]
    for n, v in SHAPES:
        vp = (v + 63) // 64 * 64
        x0 = torch.randn(n, vp, device="cuda", dtype=torch.bfloat16)
        lab = torch.randint(0, v, (n,), device="cuda")
        x = x0.clone()
        forms = {"plain": lambda: ops.softmax_xent_(x, lab, v, a.variant),
                 "options": lambda: ops.softmax_xent_opts_(x, lab, v, a.smoothing, a.z_loss, a.variant)}
        # same inputs, the expected relation between the two losses (eps = 0 would make them equal)
        ref = {}
        for k, f in forms.items():
            x.copy_(x0)
            ref[k] = f().double().mean().item()
        times = {k: [] for k in forms}
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for it in range(a.warmup + a.reps):
            for k, f in forms.items():
                x.copy_(x0)
                torch.cuda.synchronize()
                s.record()
                f()
                e.record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[k].append(s.elapsed_time(e) * 1e3)
        for k in forms:
            t = times[k]
            med = _q(t, 0.5)
            lines.append(f"{n:6d} x {v:6d} {k:8s} median {med:8.1f} us  p10 {_q(t, 0.1):8.1f}  p90 {_q(t, 0.9):8.1f}  "
                         f"{2 * n * vp * 2 / med / 1e6:6.2f} TB/s  mean loss {ref[k]:.4f}")
        d = _q(times["options"], 0.5) - _q(times["plain"], 0.5)
        lines.append(f"{n:6d} x {v:6d} options - plain: {d:+.1f} us ({100 * d / _q(times['plain'], 0.5):+.2f} %); "
                     f"plain p10-p90 spread {_q(times['plain'], 0.9) - _q(times['plain'], 0.1):.1f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
