#!/usr/bin/env python
"""Extend-attention benchmarks (needs the GPU), Llama-3-8B geometry (H 32 / Hkv 8 / D 128).  Writes a text report
(default profiles/extend_attention.txt).

    python tools/bench_extend.py                  # the kernel table and the model table
    python tools/bench_extend.py --skip_model     # the kernel table only

Kernel table: one ``fused.extend_attention`` call of T tokens per row on a cache of ``len`` tokens against the
``ceil(T / 8)`` ``fused.chunk_attention`` calls that cover the same tokens (each on the cache as it stands after
the chunks before it).  Device events around ``iters`` back-to-back calls after a warm-up, the calls rotating over
enough distinct caches that the working set exceeds the 256 MiB Infinity Cache where 8 caches suffice.

Model table: a ``--layers``-layer model of the same geometry (hidden 4096, MLP 14336; not the whole 32 layers: the
comparison is per layer) in bf16.  One extend forward of T tokens on a cache of ``len`` against ``ceil(T / 8)`` chunk
forwards, and against a fresh prefill of ``len + T`` tokens; wall time around a device synchronise."""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_lion_pytorch_amd.models import KVCache  # noqa: E402
from distributed_lion_pytorch_amd.models import llama as L  # noqa: E402
from distributed_lion_pytorch_amd.ops import fused, hip  # noqa: E402

H, HKV, D = 32, 8, 128
CACHE_BYTES = 256 << 20
TOKENS, LENGTHS, BATCHES = (16, 64, 256, 1024), (0, 1024, 8192, 32768), (1, 8)


def _time(fn, n_variants, iters, warmup=2):
    for i in range(warmup * n_variants):
        fn(i % n_variants)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i % n_variants)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def kernel_table(dev, iters, out):
    out.append(f"extend_attention against ceil(T / 8) chunk_attention calls; H {H} / Hkv {HKV} / D {D}, bf16, {iters} iterations")
    out.append(f"{'B':>2} {'len':>6} {'T':>5} {'splits':>6} {'extend us':>10} {'chunks us':>10} {'chunk calls':>11} {'ratio':>6}")
    g = torch.Generator(device=dev).manual_seed(0)
    for B in BATCHES:
        for n in LENGTHS:
            for T in TOKENS:
                tmax = n + T
                per = 2 * B * tmax * HKV * D * 2
                nv = max(1, min(8, -(-2 * CACHE_BYTES // per)))
                caches = [torch.randn(2, B, tmax, HKV, D, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(nv)]
                q = torch.randn(B, T, H, D, device=dev, dtype=torch.bfloat16, generator=g)
                base = torch.full((B,), n, dtype=torch.int32, device=dev)
                steps = [(q[:, t:t + 8].contiguous(), base + t, n + min(t + 8, T)) for t in range(0, T, 8)]
                ext = _time(lambda i: fused.extend_attention(q, caches[i][0], caches[i][1], base, None, 0, tmax), nv, iters)

                def chunks(i):
                    for qc, ln, bound in steps:
                        fused.chunk_attention(qc, caches[i][0], caches[i][1], ln, None, 0, bound)

                chk = _time(chunks, nv, max(2, iters // 4))
                s = fused.extend_splits(B, HKV, tmax, T)[0]
                out.append(f"{B:>2} {n:>6} {T:>5} {s:>6} {ext * 1e6:>10.1f} {chk * 1e6:>10.1f} {len(steps):>11} {chk / ext:>6.2f}")
                print(out[-1], flush=True)
                del caches


def model_table(dev, layers, out):
    import transformers

    cfg = transformers.LlamaConfig(vocab_size=32000, hidden_size=4096, intermediate_size=14336, num_hidden_layers=layers,
                                   num_attention_heads=H, num_key_value_heads=HKV, max_position_embeddings=40960,
                                   tie_word_embeddings=False)
    torch.manual_seed(0)
    m = L.LlamaForCausalLM(cfg).to(dev, torch.bfloat16).eval()
    base = m._decoder()
    out.append("")
    out.append(f"{layers}-layer model of the same geometry, bf16: one extend forward, ceil(T / 8) chunk forwards, a prefill of len + T")
    out.append(f"{'B':>2} {'len':>6} {'T':>5} {'extend ms':>10} {'chunks ms':>10} {'re-prefill ms':>13}")

    def wall(fn, reps=3):
        best = float("inf")
        for _ in range(reps + 1):  # the first repetition warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        return best

    with torch.no_grad():
        for B in BATCHES:
            for n in (1024, 8192):
                for T in (16, 64, 256, 1024):
                    ids = torch.randint(1, 32000, (B, n + T), device=dev)
                    cache = KVCache(cfg, B, n + T, dev, torch.bfloat16)
                    base(ids[:, :n], cache=cache)
                    keep = torch.full((B,), n, device=dev)

                    def extend():
                        cache.truncate(keep, n)
                        base(ids[:, n:], cache=cache, extend=True)

                    def chunks():
                        cache.truncate(keep, n)
                        for t in range(n, n + T, 8):
                            base(ids[:, t:t + 8], cache=cache)

                    def prefill():
                        base(ids, cache=KVCache(cfg, B, n + T, dev, torch.bfloat16))

                    out.append(f"{B:>2} {n:>6} {T:>5} {wall(extend) * 1e3:>10.2f} {wall(chunks) * 1e3:>10.2f} {wall(prefill) * 1e3:>13.2f}")
                    print(out[-1], flush=True)
                    del cache


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--skip_kernel", action="store_true")
    ap.add_argument("--skip_model", action="store_true")
    ap.add_argument("--out", default="profiles/extend_attention.txt")
    a = ap.parse_args(argv)
    hip.require()
    dev = torch.device("cuda")
    out = [f"tools/bench_extend.py on {torch.cuda.get_device_name(0)}"]
    if not a.skip_kernel:
        kernel_table(dev, a.iters, out)
    if not a.skip_model:
        model_table(dev, a.layers, out)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
