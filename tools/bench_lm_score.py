"""The read-only LM-head scoring kernel (lm_score) against the in-place loss
kernel (softmax_xent_), on the same tensors in one process, alternating call by
call; and, with --head, the whole evaluation head: predictions=True's
lm_head_score against the default path (fused loss, a second head GEMM for the
logits, argmax), on random hidden states.

    python tools/bench_lm_score.py [--head] [--reps 40] [--out FILE]

Kernel shapes: the GPT-2 bench rows (20460 x 50304), Llama-2 (8192 x 32000) and
Llama-3 (8192 x 128256), bf16.  Per form: the median device time, the p10-p90
spread and the row traffic rate (lm_score: one read of the row; softmax_xent_:
one read and one write).  Head shapes: Llama-3-8B (N 8192, C 4096, V 128256)
and GPT-2 (N 20480, C 768, V 50257)."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_lion_pytorch_amd.ops import fused, hip  # noqa: E402

SHAPES = [(20460, 50304), (8192, 32000), (8192, 128256)]
HEADS = [(8192, 4096, 128256), (20480, 768, 50257)]


def _q(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def _alternate(forms, reps, warmup, before=None):
    times = {k: [] for k in forms}
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in range(warmup + reps):
        for k, f in forms.items():
            if before is not None:
                before()
            torch.cuda.synchronize()
            s.record()
            f()
            e.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[k].append(s.elapsed_time(e) * 1e3)
    return times


def bench_kernels(a, lines):
    ops = hip.ops()
    for n, v in SHAPES:
        vp = (v + 63) // 64 * 64
        x0 = torch.randn(n, vp, device="cuda", dtype=torch.bfloat16)
        lab = torch.randint(0, v, (n,), device="cuda")
        x = x0.clone()
        forms = {"lm_score": lambda: ops.lm_score(x, lab, v, 0.0, 0.0),
                 "softmax_xent_": lambda: ops.softmax_xent_(x, lab, v, 0)}
        # same inputs: the two mean losses must agree
        loss = {"lm_score": forms["lm_score"]()[0].double().mean().item()}
        loss["softmax_xent_"] = forms["softmax_xent_"]().double().mean().item()
        times = _alternate(forms, a.reps, a.warmup, before=lambda: x.copy_(x0))
        for k, passes in (("lm_score", 1), ("softmax_xent_", 2)):
            t = times[k]
            med = _q(t, 0.5)
            lines.append(f"{n:6d} x {v:6d} {k:14s} median {med:8.1f} us  p10 {_q(t, 0.1):8.1f}  p90 {_q(t, 0.9):8.1f}  "
                         f"{passes * n * vp * 2 / med / 1e6:6.2f} TB/s  mean loss {loss[k]:.4f}")
        ms, mx = _q(times["lm_score"], 0.5), _q(times["softmax_xent_"], 0.5)
        lines.append(f"{n:6d} x {v:6d} lm_score - softmax_xent_: {ms - mx:+.1f} us ({100 * (ms - mx) / mx:+.2f} %)")
        del x, x0


def bench_heads(a, lines):
    for n, c, v in HEADS:
        h = torch.randn(n, c, device="cuda", dtype=torch.bfloat16)
        w = (0.02 * torch.randn(v, c, device="cuda")).bfloat16()
        lab = torch.randint(0, v, (n,), device="cuda")

        def default():
            loss = fused.lm_head_cross_entropy(h, w, lab)
            return loss, F.linear(h, w).argmax(-1)

        forms = {"predictions=True": lambda: fused.lm_head_score(h, w, lab), "logits + argmax": default}
        with torch.no_grad():
            s, (loss, pred) = forms["predictions=True"](), default()
            agree = (s.pred == pred).float().mean().item()
            times = _alternate(forms, a.reps, a.warmup)
        for k in forms:
            t = times[k]
            lines.append(f"head N {n:5d} C {c:4d} V {v:6d} {k:17s} median {_q(t, 0.5):9.1f} us  p10 {_q(t, 0.1):9.1f}  "
                         f"p90 {_q(t, 0.9):9.1f}")
        lines.append(f"head N {n:5d} C {c:4d} V {v:6d} loss {s.loss.item():.5f} / {loss.item():.5f}, same top-1 token "
                     f"in {100 * agree:.2f} % of the rows (two GEMMs, each rounded to bf16)")
        del h, w


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", action="store_true", help="also time the whole evaluation head")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    hip.require()
    lines = [f"# lm_score (read-only) vs softmax_xent_ (in place), {a.reps} alternating reps, bf16, "
             f"{torch.cuda.get_device_name(0)}"]
    bench_kernels(a, lines)
    if a.head:
        bench_heads(a, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
