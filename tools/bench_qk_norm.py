"""Microbenchmark of the per-head q/k RMSNorm + RoPE kernels (csrc/qk_norm.hip).

python tools/bench_qk_norm.py [--shapes 16x1024x16x8,4x2048x32x8] [--repeat 5] [--iters 100]
A shape is BxTxHxHkv at head_dim 128; q | k are the leading columns of a
[B, T, (H + 2 Hkv) 128] projection output, as in the model.  Per shape, three
things are timed in turn, --repeat times over (min..max of the rounds):

* fused   the new forward, and the new backward (in place) + the reduction of
          its gain-gradient partials;
* chain   what they replace: fused.rms_norm (the ATen chain) over the head rows
          of q and of k, then ops.rope, forward under no_grad and forward +
          backward through autograd (its backward is the difference);
* rope    plain ops.rope / ops.rope_ on the same q | k block: the same bytes
          minus rstd and without the norm.

Bandwidth is the bytes the fused kernels have to move (forward: x in, y and
rstd out; backward: g and x in, g out, rstd in, partials out) over the time,
and its share of the 8 TB/s HBM peak.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_lion_pytorch_amd.models.llama import Rotary  # noqa: E402
from distributed_lion_pytorch_amd.ops import fused, hip  # noqa: E402

D, EPS, HBM_PEAK = 128, 1e-6, 8.0e12


def timeit(fn, iters):
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


def bench(B, T, H, Hkv, repeat, iters):
    ops, dev = hip.ops(), "cuda"
    Hx = H + Hkv
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, device=dev).bfloat16()
    gbuf = torch.randn_like(qkv)
    x = qkv[..., :Hx * D].view(B, T, Hx, D)
    g = gbuf[..., :Hx * D].view(B, T, Hx, D)
    q, k = x[:, :, :H], x[:, :, H:]
    gq = torch.ones(D, device=dev).bfloat16()  # unit gains: the in-place backward, iterated, stays bounded
    gk = torch.ones(D, device=dev).bfloat16()
    cos, sin = Rotary(D, 1e6).tables(T, torch.device(dev), torch.bfloat16)
    parts = fused._qk_norm_parts(B * T)
    _, rstd = ops.qk_norm_rope_fwd(x, gq, gk, H, EPS, cos, sin)
    dz = torch.randn(B, T, Hx, D, device=dev).bfloat16()
    ql, kl = q.detach().clone().requires_grad_(), k.detach().clone().requires_grad_()
    gql, gkl = gq.clone().requires_grad_(), gk.clone().requires_grad_()

    def chain_fwd():
        with torch.no_grad():
            return fused.rope(fused.rms_norm(q, gq, EPS), cos, sin), fused.rope(fused.rms_norm(k, gk, EPS), cos, sin)

    def chain_fwd_bwd():
        zq = fused.rope(fused.rms_norm(ql, gql, EPS), cos, sin)
        zk = fused.rope(fused.rms_norm(kl, gkl, EPS), cos, sin)
        torch.autograd.backward([zq, zk], [dz[:, :, :H], dz[:, :, H:]])
        ql.grad = kl.grad = gql.grad = gkl.grad = None

    runs = {
        "fused fwd": lambda: ops.qk_norm_rope_fwd(x, gq, gk, H, EPS, cos, sin),
        "fused bwd (dz + tables) + sum": lambda: ops.sum_partials(
            ops.qk_norm_rope_bwd_(g, x, rstd, gq, gk, H, cos, sin, parts)),
        "fused bwd (dy) + sum": lambda: ops.sum_partials(ops.qk_norm_rope_bwd_(g, x, rstd, gq, gk, H, None, None, parts)),
        "chain fwd": chain_fwd,
        "chain fwd + bwd": chain_fwd_bwd,
        "rope fwd": lambda: ops.rope(x, cos, sin, False),
        "rope_ inverse (in place)": lambda: ops.rope_(g, cos, sin, True),
    }
    times = {n: [] for n in runs}
    for _ in range(repeat):  # the candidates alternate inside every round
        for n, fn in runs.items():
            times[n].append(timeit(fn, iters))
    n_el = B * T * Hx * D
    fwd_bytes = 2 * n_el * 2 + B * T * Hx * 4
    bwd_bytes = 3 * n_el * 2 + B * T * Hx * 4 + parts * 2 * D * 4
    print(f"--- B {B} T {T} heads {H}/{Hkv} D {D}: q|k block {n_el * 2 / 1e6:.1f} MB, parts {parts}")
    for n, ts in times.items():
        lo, hi = min(ts), max(ts)
        line = f"{n:32s} {lo:9.1f}..{hi:9.1f} us"
        if n.startswith("fused") or n.startswith("rope"):
            nb = fwd_bytes if "fwd" in n else bwd_bytes
            if n.startswith("rope"):
                nb = 2 * n_el * 2
            line += f"  {nb / lo / 1e3:7.1f} GB/s ({100 * nb / (lo * 1e-6) / HBM_PEAK:4.1f} % of HBM peak)"
        print(line)
    cb = [b - a for a, b in zip(times["chain fwd"], times["chain fwd + bwd"])]
    print(f"{'chain bwd (difference)':32s} {min(cb):9.1f}..{max(cb):9.1f} us")
    print(f"fused / chain: fwd {min(times['fused fwd']) / min(times['chain fwd']):.3f}, "
          f"bwd {min(times['fused bwd (dz + tables) + sum']) / min(cb):.3f} (dz + tables), "
          f"{min(times['fused bwd (dy) + sum']) / min(cb):.3f} (dy)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x1024x16x8,4x2048x32x8")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    a = ap.parse_args()
    hip.require()
    for s in a.shapes.split(","):
        bench(*(int(v) for v in s.split("x")), a.repeat, a.iters)


if __name__ == "__main__":
    main()
