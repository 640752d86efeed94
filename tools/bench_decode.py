#!/usr/bin/env python
"""Decode benchmarks (needs the GPU): the decode-attention kernel against the HBM copy rate and against the
math SDPA path, the skinny-M weight GEMMs (bf16 and 4-bit) against the same copy rate and against the general
dispatch, and end-to-end ``generate`` against the naive recompute loop, with a per-phase split of a decode
step; the LM-head top-k kernel against the PyTorch chain and beam search end to end (``--topk``,
``--num_beams``).  Writes a text report (default profiles/r13/decode.txt).

    python tools/bench_decode.py                      # everything
    python tools/bench_decode.py --skip_e2e           # the kernel tables only
    python tools/bench_decode.py --e2e gpt2           # one end-to-end model
    python tools/bench_decode.py --skip_kernel --skip_skinny --e2e llama3-4bit --ab   # skinny GEMM on / off, interleaved
    python tools/bench_decode.py --skip_kernel --skip_skinny --topk --num_beams 4 --e2e gpt2 --e2e llama3 \
        --out profiles/r14/beam.txt                   # the top-k kernel table and beam search next to greedy

Method.  Kernel times are device events around ``iters`` back-to-back calls after a warm-up, the calls rotating
over enough distinct cache buffers that the working set exceeds the 256 MiB Infinity Cache (a decode step of a
real model does the same: every layer has its own cache) -- otherwise the small shapes would be timed out of
cache.  Bytes are the K and V bytes a call has to read (B Hkv len D 2 bytes, twice), computed from the shapes; the
ceiling is the 6.29 TB/s float4-copy rate of MI355X_MICROARCH.md.  The skinny-GEMM table instead sums the kernel
durations of a profiler trace per call (its small shapes' kernels are shorter than a launch, so back-to-back calls
would time the host) and sweeps 3 x 256 MiB of distinct weights in every measurement.  End-to-end figures are wall time around a
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
from distributed_lion_pytorch_amd.ops import fused, hip, linear, quant  # noqa: E402

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


def _device_time(fn, n_variants, iters, warmup=2):
    """Seconds of kernel time per call: the summed durations of the device-side events of ``iters`` profiled
    calls (every kernel a call launches, e.g. GEMM + combine, or expansion + GEMM).  Unlike _time it does not
    see launch gaps, so it stays a kernel time where back-to-back calls are bound by the host's launch rate."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    for i in range(warmup):
        fn(i % n_variants)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for i in range(iters):
            fn((warmup + i) % n_variants)
        torch.cuda.synchronize()
    total = sum(e.time_range.elapsed_us() for e in prof.events() if e.device_type == DeviceType.CUDA)
    return total * 1e-6 / iters


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


# ------------------------------------------------------------------------------------------ skinny-M GEMMs
# [N, K] of a decode step's weight GEMMs: Llama-3-8B (q|k|v, o, gate|up, down, LM head), GPT-2 (c_attn, c_proj, c_fc,
# mlp c_proj, LM head), Qwen2-0.5B's down_proj (K = 64 x 76)
SKINNY_SHAPES = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336), (128256, 4096),
                 (2304, 768), (768, 768), (3072, 768), (768, 3072), (50257, 768), (896, 4864)]
SKINNY_M = (1, 4, 8, 16)
W4_BYTES = 0.5 + 4.0 / 64  # per weight element: two indices per byte and an fp32 absmax per 64


def skinny_table(dev, iters, shapes=SKINNY_SHAPES, rows=SKINNY_M):
    """Per shape and M: the skinny kernels' device time (kernel + combine pass where K is split over blocks),
    weight bytes / time against the copy rate, and the parent dispatch on the same operands (bf16: F.linear,
    i.e. hipBLASLt; 4-bit: expansion to bf16 + F.linear, what Linear4bit did before).  Times are summed kernel
    durations from a profiler trace (_device_time), not wall time between events: the small shapes' calls are
    shorter than a launch.  The calls rotate over 3 x 256 MiB of distinct weights, however many that takes."""
    head = (f"{'N':>6s} {'K':>5s} {'M':>2s} {'splits':>6s} | {'skinny us':>9s} {'TB/s':>5s} {'of copy':>7s} {'F.linear us':>11s} "
            f"{'speedup':>7s} | {'w4 us':>7s} {'TB/s':>5s} {'of copy':>7s} {'expand+GEMM us':>14s} {'speedup':>7s}")
    lines = [head]
    code = quant.code_tensor("nf4", dev)
    g = torch.Generator(device=dev).manual_seed(0)
    for N, K in shapes:
        wbytes = N * K * 2
        n = max(2, -(-3 * CACHE_BYTES // wbytes))
        iters = max(iters, n)  # every measurement sweeps the whole set: nothing it reads is left in the cache
        ws = [torch.randn(N, K, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(n)]
        q4 = [quant.quantize_4bit(w, code) for w in ws] if (N * K) % 64 == 0 else None
        scratch = torch.empty(N, K, device=dev, dtype=torch.bfloat16)
        for M in rows:
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16, generator=g)
            out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            splits, _ = fused.skinny_splits(M, N, K)
            t_s = _device_time(lambda i: fused.skinny_gemm(x, ws[i], out=out), n, iters)
            t_p = _device_time(lambda i: F.linear(x, ws[i]), n, iters)
            tbs = wbytes / t_s / 1e12
            row = (f"{N:6d} {K:5d} {M:2d} {splits:6d} | {t_s * 1e6:9.1f} {tbs:5.2f} {tbs / HBM_COPY_TBS:7.1%} {t_p * 1e6:11.1f} "
                   f"{t_p / t_s:6.2f}x |")
            if q4 is not None:
                t_q = _device_time(lambda i: fused.skinny_gemm_w4(x, q4[i][0], q4[i][1], code, N, out=out), n, iters)

                def expand(i):
                    return F.linear(x, quant.dequantize_4bit(q4[i][0], q4[i][1], code, (N, K), out=scratch))

                t_e = _device_time(expand, n, max(5, iters // 4))
                tbq = N * K * W4_BYTES / t_q / 1e12
                row += f" {t_q * 1e6:7.1f} {tbq:5.2f} {tbq / HBM_COPY_TBS:7.1%} {t_e * 1e6:14.1f} {t_e / t_q:6.2f}x"
            else:
                row += "  (N K is no multiple of 64: no 4-bit store)"
            lines.append(row)
            print(row, flush=True)
        del ws, q4, scratch
        torch.cuda.empty_cache()
    return lines


# ------------------------------------------------------------------------------------------ LM-head top-k
TOPK_CASES = [(N, V, k) for V in (50257, 128256) for N in (8, 16, 64) for k in (8, 64)]


def topk_table(dev, iters):
    """csrc/lm_topk.hip against the PyTorch chain a beam step would otherwise run on the same bf16 logits
    (log_softmax in fp32, then topk): summed kernel durations of a profiler trace per call (_device_time; the
    calls are shorter than a launch gap) and the bytes the chain allocates at its peak (the kernel allocates its
    three outputs, (8 k + 4) N bytes).  The logits rotate over 4 buffers that together stay inside the L2 /
    Infinity Cache: in a decode step the head GEMM has just written them."""
    lines = [f"{'N':>3s} {'V':>6s} {'k':>2s} {'kernel us':>9s} {'row read TB/s':>13s} {'chain us':>8s} {'log_softmax us':>14s} "
             f"{'topk us':>7s} {'chain / kernel':>14s} {'chain allocates':>15s}"]
    g = torch.Generator(device=dev).manual_seed(0)
    for N, V, k in TOPK_CASES:
        vp = (V + 63) // 64 * 64
        xs = [(2 * torch.randn(N, vp, device=dev, generator=g)).bfloat16() for _ in range(4)]
        t_k = _device_time(lambda i: hip.ops().lm_topk(xs[i], V, k), 4, iters)
        t_l = _device_time(lambda i: torch.log_softmax(xs[i][:, :V].float(), -1), 4, iters)
        lp = torch.log_softmax(xs[0][:, :V].float(), -1)
        t_t = _device_time(lambda i: torch.topk(lp, k, dim=-1), 4, iters)
        del lp
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = torch.topk(torch.log_softmax(xs[0][:, :V].float(), -1), k, dim=-1)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        # same selection on rows without ties at the k-th place (topk's tie order is unspecified)
        values, ids, lse = hip.ops().lm_topk(xs[0], V, k)
        same = float((values - lse[:, None] - out.values).abs().max())
        row = (f"{N:3d} {V:6d} {k:2d} {t_k * 1e6:9.1f} {N * V * 2 / t_k / 1e12:13.2f} {(t_l + t_t) * 1e6:8.1f} {t_l * 1e6:14.1f} "
               f"{t_t * 1e6:7.1f} {(t_l + t_t) / t_k:13.2f}x {peak / 2 ** 20:11.1f} MiB   max |log-prob diff| {same:.1e}")
        lines.append(row)
        print(row, flush=True)
        del xs, out
        torch.cuda.empty_cache()
    return lines


# ------------------------------------------------------------------------------------------ end to end
E2E = {"gpt2": dict(model="gpt2", B=8, prompt=128, new=256), "llama3": dict(model="llama-3-8b", B=8, prompt=512, new=256),
       "llama3-b1": dict(model="llama-3-8b", B=1, prompt=512, new=256),
       "llama3-4bit": dict(model="llama-3-8b", B=8, prompt=512, new=256, quant="nf4")}

PHASES = [("decode_attention", r"decode_attn_kernel|decode_combine_kernel"), ("kv_append", r"kv_append_kernel"),
          ("LM head scoring", r"lm_score"), ("norms", r"norm"), ("4-bit expansion", r"dequant4"),
          ("GEMMs (projections, MLP, LM head)", r"Cijk|gemm|GEMM|hipblaslt|rocblas|skinny_"),
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


def ab_decode(model, ids, steps=32, rounds=3):
    """Decode steps with the skinny GEMM routing on and off (off: the parent's dispatch, DLION_SKINNY_GEMM=0),
    the two interleaved: wall ms per step (best and worst round of each) and kernel ms per step (one profiled
    run of each)."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    cache, h = prefill(model, ids, (2 * rounds + 3) * steps * 2)
    wall = {True: [], False: []}
    kern = {}
    was = linear._SKINNY
    try:
        for on in (True, False):
            linear._SKINNY = on
            h = decode_steps(model, cache, h, steps)  # warm
        for _ in range(rounds):
            for on in (True, False):
                linear._SKINNY = on
                t, h = _wall(lambda: decode_steps(model, cache, h, steps))
                wall[on].append(t / steps * 1e3)
        for on in (True, False):
            linear._SKINNY = on
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                _, h = _wall(lambda: decode_steps(model, cache, h, steps))
            kern[on] = sum(e.time_range.elapsed_us() for e in prof.events() if e.device_type == DeviceType.CUDA) * 1e-3 / steps
    finally:
        linear._SKINNY = was
    out = []
    for on in (False, True):
        out.append(f"    skinny GEMM {'on ' if on else 'off'}: wall {min(wall[on]):.3f} .. {max(wall[on]):.3f} ms per decode step "
                   f"({rounds} rounds of {steps} steps), kernels {kern[on]:.3f} ms per step")
    out.append(f"    on / off: wall {min(wall[True]) / min(wall[False]):.3f}, kernels {kern[True] / kern[False]:.3f}")
    return out


def reorder_times(model, rows, num_beams, prompt, new, iters=50):
    """Seconds per KVCache.reorder_rows of a [rows]-row cache at generated suffixes of 1, new / 2 and new - 1
    positions above the prompt (device events around back-to-back calls)."""
    dev = model.lm_head.weight.device
    cache = KVCache(model.config, rows, prompt + new, dev, model.lm_head.weight.dtype)
    cache.prefilled = True
    index = (torch.arange(rows, device=dev) // num_beams) * num_beams + torch.randint(0, num_beams, (rows,), device=dev)
    out = []
    for suffix in (1, new // 2, new - 1):
        cache.width = prompt + suffix
        out.append((suffix, _time(lambda i: cache.reorder_rows(index, prompt), 1, iters)))
    return out


def beam_end_to_end(name, dev, num_beams):
    """Beam search at B / num_beams prompts against greedy at B rows on the same model: the decode kernels and
    the GEMMs see the same M."""
    s = E2E[name]
    cfg = load_config(s["model"])
    torch.manual_seed(0)
    with torch.device(dev):
        model = build_model(cfg, native=True).to(dtype=torch.bfloat16)
    model.eval()
    rows, Bb, new = s["B"], s["B"] // num_beams, s["new"]
    ids = torch.randint(0, cfg.vocab_size, (rows, s["prompt"]), device=dev)
    kw = dict(num_beams=num_beams, num_return_sequences=num_beams)
    lines = [f"{s['model']}: {s['prompt']} prompt + {new} new tokens, bf16, random weights; beam search B = {Bb} x "
             f"{num_beams} beams against greedy B = {rows} ({rows} rows per decode step either way)"]
    model.generate(ids, max_new_tokens=8)
    model.generate(ids[:Bb], max_new_tokens=8, **kw)  # warm-up: code objects, GEMM algorithm choices
    per = {}
    for rnd in range(2):  # the two alternate; the better round of each is reported, both are printed
        for what, call in (("greedy", lambda n: model.generate(ids, max_new_tokens=n)),
                           ("beam", lambda n: model.generate(ids[:Bb], max_new_tokens=n, **kw))):
            t, out = _wall(lambda: call(new))
            assert out.shape == (rows, s["prompt"] + new), out.shape
            t1, _ = _wall(lambda: call(1))
            per.setdefault(what, []).append((t - t1) / (new - 1) * 1e3)
            lines.append(f"  round {rnd} {what:6s}: {t:.3f} s, prefill + first token {t1 * 1e3:.1f} ms, "
                         f"{per[what][-1]:.3f} ms per step")
    g, b = min(per["greedy"]), min(per["beam"])
    lines.append(f"  ms per step: beam {b:.3f}, greedy {g:.3f}, beam / greedy {b / g:.3f}")
    for suffix, t in reorder_times(model, rows, num_beams, s["prompt"], new):
        lines.append(f"  reorder_rows at a suffix of {suffix:3d} positions: {t * 1e6:8.1f} us, {t * 1e3 / b:6.1%} of a beam step")
    del model
    torch.cuda.empty_cache()
    return lines


def end_to_end(name, dev, naive_steps, ab=False):
    s = E2E[name]
    cfg = load_config(s["model"])
    torch.manual_seed(0)
    with torch.device(dev):
        model = build_model(cfg, native=True).to(dtype=torch.bfloat16)
    if s.get("quant"):
        from distributed_lion_pytorch_amd.models.quant import quantize_model

        quantize_model(model, bnb_4bit_quant_type=s["quant"])
    model.eval()
    ids = torch.randint(0, cfg.vocab_size, (s["B"], s["prompt"]), device=dev)
    lines = [f"{s['model']}: B = {s['B']}, {s['prompt']} prompt + {s['new']} new tokens, bf16"
             f"{', ' + s['quant'] + ' base' if s.get('quant') else ''}, random weights, greedy"]
    model.generate(ids, max_new_tokens=8)  # warm-up: code objects, GEMM algorithm choices
    if ab:
        lines += ab_decode(model, ids)
        del model
        torch.cuda.empty_cache()
        return lines
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
    ap.add_argument("--out", default=os.path.join("profiles", "r13", "decode.txt"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--skip_kernel", action="store_true")
    ap.add_argument("--skip_skinny", action="store_true")
    ap.add_argument("--ab", action="store_true",
                    help="end to end: decode steps with the skinny GEMM routing on and off, interleaved, instead of "
                         "the generate / naive-loop / phase report")
    ap.add_argument("--skip_e2e", action="store_true")
    ap.add_argument("--e2e", action="append", choices=sorted(E2E), default=None)
    ap.add_argument("--naive_steps", type=int, default=16)
    ap.add_argument("--topk", action="store_true", help="the LM-head top-k kernel table (csrc/lm_topk.hip)")
    ap.add_argument("--num_beams", type=int, default=1,
                    help="end to end: beam search at B / num_beams prompts next to greedy at B rows, instead of the "
                         "generate / naive-loop / phase report")
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
    if not a.skip_skinny:
        head = ["## skinny-M GEMM (csrc/skinny_gemm.hip), weight bytes over device time (summed kernel durations of a "
                f"profiler trace) against the {HBM_COPY_TBS} TB/s float4 copy; 4-bit bytes are {W4_BYTES} per element", ""]
        print("\n".join(head), flush=True)
        report += head + skinny_table(dev, a.iters) + [""]
    if a.topk:
        head = ["## LM-head top-k (csrc/lm_topk.hip) against log_softmax (fp32) + topk on the same bf16 logits; device "
                "time = summed kernel durations of a profiler trace", ""]
        print("\n".join(head), flush=True)
        report += head + topk_table(dev, a.iters) + [""]
    if not a.skip_e2e:
        report += ["## end to end", ""]
        for name in a.e2e or sorted(E2E):
            if a.num_beams > 1:
                lines = beam_end_to_end(name, dev, a.num_beams)
            else:
                lines = end_to_end(name, dev, a.naive_steps, a.ab)
            print("\n".join(lines), flush=True)
            report += lines + [""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(report))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
