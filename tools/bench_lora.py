"""Timings of the LoRA streams (csrc/lora.hip, csrc/lora_wide.hip) at the
Llama-2-7B LoRA SFT shape: 4096 tokens, K = N = 4096, o / dout as column views
of a fused q|k|v projection output (row stride 12288).

Default: each kernel on its own, us and the effective HBM bandwidth of its
compulsory traffic.  ``--op``: the whole adapter op, forward + backward
(ops/fused.lora_add on leaf tensors), fused against the unfused ATen chain
(``fused._LORA_FUSED = False``) on the same tensors in one process, the two
alternating over ``--rounds`` rounds; prints every round and the medians."""
import argparse
import statistics

import torch

from distributed_lion_pytorch_amd.ops import fused, hip


def timeit(fn, iters=50):
    for _ in range(5):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def bench_op(M, K, N, r, p, rounds, iters):
    """Forward + backward of the adapter op, fused and unfused alternating."""
    dev = "cuda"
    x = torch.randn(M, K, device=dev, dtype=torch.bfloat16).requires_grad_()
    wide = torch.randn(M, 3 * N, device=dev, dtype=torch.bfloat16)
    o = wide[:, :N].detach().requires_grad_()
    dwide = torch.randn(M, 3 * N, device=dev, dtype=torch.bfloat16)
    dout = dwide[:, :N]
    A = (torch.randn(r, K, device=dev) * 0.05).to(torch.bfloat16).requires_grad_()
    B = (torch.randn(N, r, device=dev) * 0.05).to(torch.bfloat16).requires_grad_()
    calls = []
    real = fused._LoraAdd.forward
    fused._LoraAdd.forward = staticmethod(lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])

    def step():
        for t in (x, o, A, B):
            t.grad = None
        fused.lora_add(o, x, A, B, 2.0, p).backward(dout)

    def run(flag):
        fused._LORA_FUSED = flag
        n0 = len(calls)
        us = timeit(step, iters)
        assert (len(calls) > n0) == flag, "the fused switch did not select the path"
        return us

    series = {True: [], False: []}
    for i in range(rounds):
        for flag in (True, False):
            series[flag].append(run(flag))
        print(f"  round {i}: fused {series[True][-1]:8.1f} us   unfused {series[False][-1]:8.1f} us", flush=True)
    fused._LORA_FUSED = True
    fused._LoraAdd.forward = staticmethod(real)
    mf, mu = statistics.median(series[True]), statistics.median(series[False])
    print(f"op fwd+bwd M={M} K={K} N={N} r={r} p={p}: fused median {mf:.1f} us (min {min(series[True]):.1f}, max "
          f"{max(series[True]):.1f}), unfused median {mu:.1f} us (min {min(series[False]):.1f}, max "
          f"{max(series[False]):.1f}), unfused / fused {mu / mf:.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--r", type=int, default=8)
    ap.add_argument("--op", action="store_true", help="time the whole op forward + backward, fused against unfused")
    ap.add_argument("--p", type=float, default=0.05, help="adapter dropout of --op")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    hip.require()
    ops = hip.ops()
    M, K, N, r = a.tokens, a.k, a.n, a.r
    if a.op:
        bench_op(M, K, N, r, a.p, a.rounds, a.iters)
        return
    dev = "cuda"
    x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
    wide = torch.randn(M, 3 * N, device=dev, dtype=torch.bfloat16)
    o = wide[:, :N]
    A = torch.randn(r, K, device=dev, dtype=torch.bfloat16) * 0.05
    B = torch.randn(N, r, device=dev, dtype=torch.bfloat16) * 0.05
    u = ops.lora_rows(x, A, 1.0, 0.05, 1)
    du = ops.lora_rows(o, B.t().contiguous(), 2.0, 0.0, 0)
    mb = 1 << 20
    rows = [
        ("rows down (drop)", lambda: ops.lora_rows(x, A, 1.0, 0.05, 1), M * K * 2),
        ("rows du", lambda: ops.lora_rows(o, B.t().contiguous(), 2.0, 0.0, 0), M * N * 2),
        ("up", lambda: ops.lora_up(o, u, B, 2.0), 2 * M * N * 2),
        ("cols dB", lambda: ops.lora_cols(o, u, None, 2.0, 0.0, 0), M * N * 2),
        ("cols dA+dx", lambda: ops.lora_cols(x, du, A, 1.0, 0.05, 1), 2 * M * K * 2),
    ]
    calib = [("copy strided o", lambda: o.contiguous(), 2 * M * N * 2), ("clone x", lambda: x.clone(), 2 * M * K * 2),
             ("sum x (read)", lambda: x.sum(), M * K * 2)]
    print(f"kernels M={M} K={K} N={N} r={r}")
    tot = 0.0
    for name, fn, nbytes in rows:
        us = timeit(fn, a.iters)
        tot += us
        print(f"{name:18s} {us:8.1f} us  {nbytes / mb:6.0f} MB  {nbytes / us / 1e6:5.2f} TB/s", flush=True)
    print(f"{'total':18s} {tot:8.1f} us")
    for name, fn, nbytes in calib:
        us = timeit(fn, a.iters)
        print(f"{name:18s} {us:8.1f} us  {nbytes / mb:6.0f} MB  {nbytes / us / 1e6:5.2f} TB/s  (ATen calibration)")


if __name__ == "__main__":
    main()
