"""Microbenchmark of the fused add+norm kernels (GPT-2 bench shape by default).

python tools/bench_norm.py [--rows 20480] [--C 768,896] [--rms] [--p 0.1] [--parts 128,256,512,1024]
                           [--repeat 3] [--iters 200] [--no-gelu]
For each width: per-call time and effective HBM bandwidth of add_norm_fwd /
add_norm_bwd (+ the partial reduction), then fused.dropout_add_norm forward +
backward against its own ATen fallback branch (set_impl("torch")) on the same
tensors, the two alternated in this process.  Every timing is taken --repeat
times and printed as min..max.  bias_gelu fwd/bwd follows unless --no-gelu.
"""
import argparse

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_lion_pytorch_amd.ops import fused, hip


ITERS = 200  # --iters: a timed window of 200 calls is 5-50 ms at these shapes


def timeit(fn, iters=None):
    iters = iters or ITERS
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def spread(fn, repeat):
    ts = [timeit(fn) for _ in range(repeat)]
    return min(ts), max(ts)


def fmt(mm):
    return f"{mm[0]:8.1f}..{mm[1]:8.1f} us"


def bench_width(ops, R, C, rms, p, parts_list, repeat):
    dev = "cuda"
    x = torch.randn(R, C, device=dev, dtype=torch.bfloat16)
    y = torch.randn_like(x)
    g = torch.ones(C, device=dev, dtype=torch.bfloat16)
    b = torch.zeros_like(g)
    beta = None if rms else b
    kind = "exact" if C in fused.NORM_WIDTHS else "tail"
    print(f"--- rows {R} C {C} ({kind}) {'RMS' if rms else 'LN'} p {p}")
    xo, h, mean, rstd = ops.add_norm_fwd(x, y, b, g, beta, 1e-5, rms, p, 7)
    t = spread(lambda: ops.add_norm_fwd(x, y, b, g, beta, 1e-5, rms, p, 7), repeat)
    print(f"add_norm_fwd   {fmt(t)}  {4 * R * C * 2 / t[0] / 1e3:7.1f} GB/s")
    dh, dxo = torch.randn_like(x), torch.randn_like(x)
    for parts in parts_list or [fused._norm_parts(R, C)]:
        t = spread(lambda: ops.add_norm_bwd(dh, dxo, xo, g, mean, rstd, rms, p, 7, True, parts), repeat)
        t2 = spread(lambda: ops.sum_partials(ops.add_norm_bwd(dh, dxo, xo, g, mean, rstd, rms, p, 7, True, parts)[2]),
                    repeat)
        print(f"add_norm_bwd parts={parts:5d} {fmt(t)}  {5 * R * C * 2 / t[0] / 1e3:7.1f} GB/s   +sum {fmt(t2)}")

    # the public op, forward + backward, against its own ATen fallback branch
    ys, xs = y.clone().requires_grad_(), x.clone().requires_grad_()
    gs = g.clone().requires_grad_()
    bs = None if rms else b.clone().requires_grad_()

    def step(mode):
        fused.set_impl(mode)
        xo_, h_ = fused.dropout_add_norm(ys, xs, gs, bs, 1e-5, p, rms=rms)
        torch.autograd.backward([xo_, h_], [dxo, dh])
        ys.grad = xs.grad = gs.grad = None
        if bs is not None:
            bs.grad = None

    mode0 = fused.get_impl()
    try:
        tf, ta = [], []
        for _ in range(repeat):  # alternated: both see the same clocks and cache state
            tf.append(timeit(lambda: step(mode0)))
            ta.append(timeit(lambda: step("torch")))
    finally:
        fused.set_impl(mode0)
    print(f"fwd+bwd fused  {fmt((min(tf), max(tf)))}   ATen composite {fmt((min(ta), max(ta)))}   "
          f"ATen/fused {min(ta) / min(tf):5.2f}x")


def main():
    global ITERS
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20480)
    ap.add_argument("--C", default="768", help="comma list of row widths")
    ap.add_argument("--rms", action="store_true", help="RMSNorm instead of LayerNorm")
    ap.add_argument("--p", type=float, default=0.1, help="dropout probability of the branch")
    ap.add_argument("--parts", default="64,128,256,512,1024,2048",
                    help="backward partial counts to sweep; empty = the one ops/fused.py picks")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--iters", type=int, default=ITERS, help="calls per timed window")
    ap.add_argument("--no-gelu", action="store_true", help="skip the bias_gelu section")
    a = ap.parse_args()
    ITERS = a.iters
    ops = hip.ops()
    dev = "cuda"
    R = a.rows
    widths = [int(v) for v in a.C.split(",")]
    parts_list = [int(v) for v in a.parts.split(",") if v]
    for C in widths:
        bench_width(ops, R, C, a.rms, a.p, parts_list, a.repeat)
    if a.no_gelu:
        return
    C = widths[0]
    N = 4 * C
    z = torch.randn(R, N, device=dev, dtype=torch.bfloat16)
    bb = torch.zeros(N, device=dev, dtype=torch.bfloat16)
    t = timeit(lambda: ops.bias_gelu_fwd(z, bb, False))
    print(f"bias_gelu_fwd  {t:8.1f} us  {2 * R * N * 2 / t / 1e3:7.1f} GB/s")
    dz = torch.randn_like(z)
    for p in (256, 1024, 2560):
        t = timeit(lambda: ops.bias_gelu_bwd(dz, z, bb, False, p))
        t2 = timeit(lambda: ops.sum_partials(ops.bias_gelu_bwd(dz, z, bb, False, p)[1]))
        print(f"bias_gelu_bwd parts={p:5d} {t:8.1f} us  {3 * R * N * 2 / t / 1e3:7.1f} GB/s   +sum {t2:8.1f} us")


if __name__ == "__main__":
    main()
