#!/usr/bin/env python
"""Decode benchmarks (needs the GPU): the decode-attention kernel against the HBM copy rate and against the
math SDPA path, and end-to-end ``generate`` against the naive recompute loop, with a per-phase split of a decode
step.  Writes a text report (default profiles/r12/decode.txt).

    python tools/bench_decode.py                      # everything
    python tools/bench_decode.py --skip_e2e           # the kernel table only
    python tools/bench_decode.py --e2e gpt2           # one end-to-end model

Method.  Kernel times are device events around ``iters`` back-to-back calls after a warm-up, the calls rotating
over enough distinct cache buffers that the working set exceeds the 256 MiB Infinity Cache (a decode step of a
real model does the same: every layer has its own cache) -- otherwise the small shapes would be timed out of
cache.  Bytes are the K and V bytes a call has to read (B Hkv len D 2 bytes, twice), computed from the shapes; the
ceiling is the 6.29 TB/s float4-copy rate of MI355X_MICROARCH.md.  End-to-end figures are wall time around a
device synchronise, profiler off; the phase split comes from a separate, profiled run of 16 decode steps after the prefill.
"""
from __future__ import annotations

import argparse
import os
import re
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_lion_pytorch_amd.models import KVCache  # noqa: E402
from distributed_lion_pytorch_amd.models.registry import build_model, load_config  # noqa: E402
from distributed_lion_pytorch_amd.ops import fused, hip  # noqa: E402

HBM_COPY_TBS = 6.29  # MI355X_MICROARCH.md: float4 copy
CACHE_BYTES = 256 << 20

KERNEL_SHAPES = [(B, 32, 8, 128, L) for L in (2048, 8192) for B in (1, 8, 32)] + [(B, 12, 12, 64, 1024) for B in (1, 8, 32)]


def _time(fn, n_variants, iters, warmup=3):
    for i in range(warmup * min(n_variants, 4)):
        fn(i % n_variants)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i % n_variants)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def kernel_table(dev, iters):
    from torch.nn.attention import SDPBackend, sdpa_kernel

    lines = [f"{'B':>3s} {'H':>3s} {'Hkv':>3s} {'D':>4s} {'len':>5s} {'splits':>6s} {'kernel us':>10s} {'K+V TB/s':>9s} "
             f"{'of copy':>8s} {'math us':>9s} {'torch-form us':>13s} {'speedup':>8s}"]
    for B, H, Hkv, D, L in KERNEL_SHAPES:
        kv_bytes = 2 * B * Hkv * L * D * 2
        n = max(2, min(64, -(-3 * CACHE_BYTES // kv_bytes)))
        g = torch.Generator(device=dev).manual_seed(0)
        caches = [torch.randn(2, B, L, Hkv, D, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(n)]
        q = torch.randn(B, H, D, device=dev, dtype=torch.bfloat16, generator=g)
        kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
        splits, _ = fused.decode_splits(B, Hkv, L)
        t_k = _time(lambda i: fused.decode_attention(q, caches[i][0], caches[i][1], kv_len, 0, L), n, iters)
        rep = H // Hkv
        q4 = q[:, :, None, :]

        def math(i):  # the backend fused._sdpa_math runs, on the same cache contents (every key visible)
            k, v = caches[i][0].transpose(1, 2), caches[i][1].transpose(1, 2)
            if rep > 1:
                k, v = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
            with sdpa_kernel([SDPBackend.MATH]):
                return F.scaled_dot_product_attention(q4, k, v)

        m_iters = max(5, iters // 10)
        t_m = _time(math, n, m_iters)
        t_t = _time(lambda i: fused.decode_attention_reference(q, caches[i][0], caches[i][1], kv_len, 0, L), n, m_iters)
        # same contents, same answer (bf16 outputs of two different summation orders)
        a = fused.decode_attention(q, caches[0][0], caches[0][1], kv_len, 0, L).float()
        r = math(0).reshape(B, H * D).float()
        err = float((a - r).abs().max())
        tbs = kv_bytes / t_k / 1e12
        lines.append(f"{B:3d} {H:3d} {Hkv:3d} {D:4d} {L:5d} {splits:6d} {t_k * 1e6:10.1f} {tbs:9.2f} {tbs / HBM_COPY_TBS:8.1%} "
                     f"{t_m * 1e6:9.1f} {t_t * 1e6:13.1f} {min(t_m, t_t) / t_k:7.1f}x   max |kernel - math| {err:.1e}")
        del caches
        torch.cuda.empty_cache()
    return lines


# ------------------------------------------------------------------------------------------ end to end
E2E = {"gpt2": dict(model="gpt2", B=8, prompt=128, new=256), "llama3": dict(model="llama-3-8b", B=8, prompt=512, new=256)}

PHASES = [("decode_attention", r"decode_attn_kernel|decode_combine_kernel"), ("kv_append", r"kv_append_kernel"),
          ("LM head scoring", r"lm_score"), ("norms", r"norm"), ("GEMMs (projections, MLP, LM head)", r"Cijk|gemm|GEMM|hipblaslt|rocblas"),
          ("activation / elementwise / copies", r"swiglu|gelu|elementwise|vectorized|rope|embed|index|copy|Memcpy|Memset|fill")]


@torch.no_grad()
def prefill(model, ids, room):
    """(cache, last hidden state) after the prompt, with room for ``room`` decode steps."""
    B, T = ids.shape
    cache = KVCache(model.config, B, T + room, ids.device, model.lm_head.weight.dtype)
    return cache, model._decoder()(ids, cache=cache)[:, -1]


@torch.no_grad()
def decode_steps(model, cache, h, steps):
    """Greedy decode steps with the cache API (what generate's loop does, without EOS handling)."""
    base = model._decoder()
    ignore = torch.full((h.shape[0],), -100, dtype=torch.long, device=h.device)
    for _ in range(steps):
        tok = fused.lm_head_score(h, model.lm_head.weight, ignore).pred.long()
        h = base(tok[:, None], cache=cache)[:, 0]
    return h


@torch.no_grad()
def naive_loop(model, ids, steps):
    for _ in range(steps):
        h = model._decoder()(ids)[:, -1]
        tok = F.linear(h, model.lm_head.weight).argmax(-1, keepdim=True)
        ids = torch.cat([ids, tok], dim=1)
    return ids


def _wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def phase_split(model, ids, steps=32):
    from torch.profiler import ProfilerActivity, profile

    cache, h = prefill(model, ids, 2 * steps)
    h = decode_steps(model, cache, h, steps)  # warm
    t_plain, _ = _wall(lambda: decode_steps(model, cache, h, steps // 2))
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        wall, _ = _wall(lambda: decode_steps(model, cache, h, steps // 2))
    steps = steps // 2
    from torch.autograd import DeviceType

    per_kernel = {}  # device-side events only: an operator's device time is its kernels' and would count twice
    for e in prof.events():
        if e.device_type == DeviceType.CUDA:
            per_kernel[e.name] = per_kernel.get(e.name, 0.0) + e.time_range.elapsed_us()
    rows = [(k, t) for k, t in per_kernel.items() if t > 0]
    total = sum(t for _, t in rows)
    acc = {name: 0.0 for name, _ in PHASES}
    acc["other kernels"] = 0.0
    for k, t in rows:
        for name, pat in PHASES:
            if re.search(pat, k):
                acc[name] += t
                break
        else:
            acc["other kernels"] += t
    out = [f"  {steps} decode steps after the prefill: {t_plain * 1e3:.1f} ms wall with the profiler off, {wall * 1e3:.1f} ms under it, "
           f"{total * 1e-3:.1f} ms of kernels"]
    for name, t in acc.items():
        out.append(f"    {name:36s} {t * 1e-3:9.2f} ms {t / max(total, 1e-9):7.1%} of kernel time")
    out.append(f"    {'host gaps (profiler-off wall - kernels)':36s} {t_plain * 1e3 - total * 1e-3:9.2f} ms "
               f"({max(0.0, 1 - total * 1e-6 / t_plain):.0%} of the wall time)")
    top = sorted(rows, key=lambda r: -r[1])[:6]
    out += [f"    top kernel: {t * 1e-3:8.2f} ms  {k[:110]}" for k, t in top]
    return out


def end_to_end(name, dev, naive_steps):
    s = E2E[name]
    cfg = load_config(s["model"])
    torch.manual_seed(0)
    with torch.device(dev):
        model = build_model(cfg, native=True).to(dtype=torch.bfloat16)
    model.eval()
    ids = torch.randint(0, cfg.vocab_size, (s["B"], s["prompt"]), device=dev)
    lines = [f"{s['model']}: B = {s['B']}, {s['prompt']} prompt + {s['new']} new tokens, bf16, random weights, greedy"]
    model.generate(ids, max_new_tokens=8)  # warm-up: code objects, GEMM algorithm choices
    t, out = _wall(lambda: model.generate(ids, max_new_tokens=s["new"]))
    assert out.shape[1] == s["prompt"] + s["new"]
    t_pre, _ = _wall(lambda: model.generate(ids, max_new_tokens=1))
    n = s["B"] * s["new"]
    lines.append(f"  generate: {t:.3f} s, {n / t:.0f} tokens/s  (prefill + first token {t_pre * 1e3:.1f} ms; "
                 f"{(t - t_pre) / (s['new'] - 1) * 1e3:.2f} ms per decode step)")
    naive_loop(model, ids, 2)
    tn, _ = _wall(lambda: naive_loop(model, ids, naive_steps))
    lines.append(f"  naive recompute loop, first {naive_steps} new tokens only (it slows down as the sequence grows): "
                 f"{tn:.3f} s, {s['B'] * naive_steps / tn:.0f} tokens/s")
    try:
        lines += phase_split(model, ids)
    except Exception as e:  # the profiler is optional: the timed figures above do not depend on it
        lines.append(f"  phase split: not measured ({type(e).__name__}: {e})")
    del model
    torch.cuda.empty_cache()
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "r12", "decode.txt"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--skip_kernel", action="store_true")
    ap.add_argument("--skip_e2e", action="store_true")
    ap.add_argument("--e2e", action="append", choices=sorted(E2E), default=None)
    ap.add_argument("--naive_steps", type=int, default=16)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode.py measures on the GPU; there is none here")
    hip.require()
    dev = torch.device("cuda", 0)
    report = [f"# tools/bench_decode.py on {torch.cuda.get_device_name(0)}", ""]
    if not a.skip_kernel:
        report += ["## decode_attention, bf16, every row at full length; K+V bytes over kernel time against the "
                   f"{HBM_COPY_TBS} TB/s float4 copy", ""] + kernel_table(dev, a.iters) + [""]
        print("\n".join(report), flush=True)
    if not a.skip_e2e:
        report += ["## end to end", ""]
        for name in a.e2e or sorted(E2E):
            lines = end_to_end(name, dev, a.naive_steps)
            print("\n".join(lines), flush=True)
            report += lines + [""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(report))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
