#!/usr/bin/env python
"""Extend-attention benchmarks (needs the GPU), Llama-3-8B geometry (H 32 / Hkv 8 / D 128).  Writes a text report
(default profiles/extend_attention.txt).

    python tools/bench_extend.py                  # the kernel table and the model table
    python tools/bench_extend.py --skip_model     # the kernel table only
    python tools/bench_extend.py --fp8 --out profiles/kv8_extend.txt    # both tables on an fp8 (e4m3) KV cache

Kernel table: one ``fused.extend_attention`` call of T tokens per row on a cache of ``len`` tokens against the
``ceil(T / 8)`` ``fused.chunk_attention`` calls that cover the same tokens (each on the cache as it stands after
the chunks before it).  Device events around ``iters`` back-to-back calls after a warm-up, the calls rotating over
enough distinct caches that the working set exceeds the 256 MiB Infinity Cache where 8 caches suffice.

Model table: a ``--layers``-layer model of the same geometry (hidden 4096, MLP 14336; not the whole 32 layers: the
comparison is per layer) in bf16.  One extend forward of T tokens on a cache of ``len`` against ``ceil(T / 8)`` chunk
forwards, and against a fresh prefill of ``len + T`` tokens; wall time around a device synchronise.

``--fp8``: the same shapes on an fp8 cache.  Kernel table: ``fused.cached_attention_fp8`` (csrc/kv8_extend_attention.hip)
against the PyTorch form that served T > 8 before that kernel (``fused.cached_attention_fp8_reference``; left out, "-",
where its [B, T, H, L] fp32 scores alone exceed ``REF_SCORE_BYTES``) and against ``fused.extend_attention`` on a bf16
cache of the same shape.  Model table: one extend forward on an fp8 cache against the same forward with the append and
the attention of T > 8 tokens routed to their PyTorch forms."""
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
REF_SCORE_BYTES = 4 << 30
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


def _fp8_cache(B, tmax, dev, g):
    """Random finite e4m3 codes [2, B, tmax, HKV, D] and power-of-two scales [2, B, tmax, HKV] (|value| < 2)."""
    codes = torch.randint(0, 256, (2, B, tmax, HKV, D), device=dev, dtype=torch.uint8, generator=g)
    codes = torch.where((codes & 0x7F) == 0x7F, torch.full_like(codes, 0x38), codes)  # no NaN codes
    scales = torch.exp2(torch.randint(-10, -7, (2, B, tmax, HKV), device=dev, generator=g).float())
    return codes, scales


def kernel_table_fp8(dev, iters, out):
    out.append(f"cached_attention_fp8 (T > 8: kv8_extend_attention.hip) against its PyTorch form and against extend_attention "
               f"on a bf16 cache; H {H} / Hkv {HKV} / D {D}, {iters} iterations")
    out.append(f"{'B':>2} {'len':>6} {'T':>5} {'splits':>6} {'fp8 us':>10} {'torch us':>11} {'torch/fp8':>9} {'bf16 us':>10} {'fp8/bf16':>8}")
    g = torch.Generator(device=dev).manual_seed(0)
    for B in BATCHES:
        for n in LENGTHS:
            for T in TOKENS:
                tmax = n + T
                per = 2 * B * tmax * HKV * (D + 4)
                nv = max(1, min(8, -(-2 * CACHE_BYTES // per)))
                c8 = [_fp8_cache(B, tmax, dev, g) for _ in range(nv)]
                q = torch.randn(B, T, H, D, device=dev, dtype=torch.bfloat16, generator=g)
                base = torch.full((B,), n, dtype=torch.int32, device=dev)

                def fp8(i, fn=fused.cached_attention_fp8):
                    (kc, vc), (ks, vs) = c8[i]
                    return fn(q, kc, ks, vc, vs, base, None, 0, tmax)

                new = _time(fp8, nv, iters)
                ref = None
                if B * T * H * tmax * 4 <= REF_SCORE_BYTES:
                    ref = _time(lambda i: fp8(i, fused.cached_attention_fp8_reference), nv, max(2, iters // 10), warmup=1)
                del c8
                nv16 = max(1, min(8, -(-2 * CACHE_BYTES // (2 * B * tmax * HKV * D * 2))))
                c16 = [torch.randn(2, B, tmax, HKV, D, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(nv16)]
                b16 = _time(lambda i: fused.extend_attention(q, c16[i][0], c16[i][1], base, None, 0, tmax), nv16, iters)
                del c16
                s = fused.extend_splits(B, HKV, tmax, T)[0]
                rt = ("-", "-") if ref is None else (f"{ref * 1e6:.1f}", f"{ref / new:.1f}")
                out.append(f"{B:>2} {n:>6} {T:>5} {s:>6} {new * 1e6:>10.1f} {rt[0]:>11} {rt[1]:>9} {b16 * 1e6:>10.1f} {new / b16:>8.2f}")
                print(out[-1], flush=True)


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


class _torch_forms_above_8:
    """What an fp8 cache ran for T > 8 before the fp8 extend kernel: the PyTorch forms of the append and the attention."""

    def __enter__(self):
        self.saved = fused.kv_append_chunk, fused.cached_attention_fp8

        def append(q, k, v, pos, cos, sin, qg, kg, eps, kc, vc, n_new=None, ks=None, vs=None):
            if q.shape[1] > fused.CHUNK_MAX_TOKENS and ks is not None:
                return fused.kv_append_chunk_reference(q, k, v, pos, cos, sin, qg, kg, eps, kc, vc, n_new, ks, vs)
            return self.saved[0](q, k, v, pos, cos, sin, qg, kg, eps, kc, vc, n_new, ks, vs)

        def attend(q, kc, ks, vc, vs, kv_len, n_new=None, window=0, max_len=None, splits=None):
            if q.shape[1] > fused.CHUNK_MAX_TOKENS:
                return fused.cached_attention_fp8_reference(q, kc, ks, vc, vs, kv_len, n_new, window, max_len)
            return self.saved[1](q, kc, ks, vc, vs, kv_len, n_new, window, max_len, splits)

        fused.kv_append_chunk, fused.cached_attention_fp8 = append, attend

    def __exit__(self, *exc):
        fused.kv_append_chunk, fused.cached_attention_fp8 = self.saved


def model_table_fp8(dev, layers, out):
    import transformers

    cfg = transformers.LlamaConfig(vocab_size=32000, hidden_size=4096, intermediate_size=14336, num_hidden_layers=layers,
                                   num_attention_heads=H, num_key_value_heads=HKV, max_position_embeddings=40960,
                                   tie_word_embeddings=False)
    torch.manual_seed(0)
    m = L.LlamaForCausalLM(cfg).to(dev, torch.bfloat16).eval()
    base = m._decoder()
    out.append("")
    out.append(f"{layers}-layer model of the same geometry, bf16 on an fp8 cache: one extend forward through the kernels, the same "
               f"forward with the PyTorch forms of the append and the attention, and the kernels on a bf16 cache")
    out.append(f"{'B':>2} {'len':>6} {'T':>5} {'fp8 ms':>10} {'torch ms':>10} {'torch/fp8':>9} {'bf16 ms':>10}")

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
                    keep = torch.full((B,), n, device=dev)
                    times = []
                    for kv_dtype, parent in (("fp8_e4m3", False), ("fp8_e4m3", True), (None, False)):
                        cache = KVCache(cfg, B, n + T, dev, torch.bfloat16, kv_dtype)
                        base(ids[:, :n], cache=cache)

                        def extend():
                            cache.truncate(keep, n)
                            base(ids[:, n:], cache=cache, extend=True)

                        if parent:
                            with _torch_forms_above_8():
                                times.append(wall(extend, reps=2))
                        else:
                            times.append(wall(extend))
                        del cache
                    new, old, b16 = times
                    out.append(f"{B:>2} {n:>6} {T:>5} {new * 1e3:>10.2f} {old * 1e3:>10.2f} {old / new:>9.1f} {b16 * 1e3:>10.2f}")
                    print(out[-1], flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--skip_kernel", action="store_true")
    ap.add_argument("--skip_model", action="store_true")
    ap.add_argument("--fp8", action="store_true", help="the tables on an fp8 (e4m3) KV cache")
    ap.add_argument("--out", default="profiles/extend_attention.txt")
    a = ap.parse_args(argv)
    hip.require()
    dev = torch.device("cuda")
    out = [f"tools/bench_extend.py on {torch.cuda.get_device_name(0)}"]
    if not a.skip_kernel:
        (kernel_table_fp8 if a.fp8 else kernel_table)(dev, a.iters, out)
    if not a.skip_model:
        (model_table_fp8 if a.fp8 else model_table)(dev, a.layers, out)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
