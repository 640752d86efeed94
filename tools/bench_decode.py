#!/usr/bin/env python
"""Decode benchmarks (needs the GPU): the decode-attention kernel against the HBM copy rate and against the
math SDPA path, the skinny-M weight GEMMs (bf16 and 4-bit) against the same copy rate and against the general
dispatch, and end-to-end ``generate`` against the naive recompute loop, with a per-phase split of a decode
step; the LM-head top-k kernel against the PyTorch chain and beam search end to end (``--topk``,
``--num_beams``); the LM-head sampling kernel against the warp / multinomial chain (``--sample``).  Writes a text report (default profiles/r13/decode.txt).

    python tools/bench_decode.py                      # everything
    python tools/bench_decode.py --skip_e2e           # the kernel tables only
    python tools/bench_decode.py --e2e gpt2           # one end-to-end model
    python tools/bench_decode.py --skip_kernel --skip_skinny --e2e llama3-4bit --ab   # skinny GEMM on / off, interleaved
    python tools/bench_decode.py --skip_kernel --skip_skinny --topk --num_beams 4 --e2e gpt2 --e2e llama3 \
        --out profiles/r14/beam.txt                   # the top-k kernel table and beam search next to greedy
    python tools/bench_decode.py --skip_kernel --skip_skinny --skip_e2e --sample --out profiles/lm_sample.txt

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


def kv8_table(dev, iters, chunks=(1, 5, 8)):
    """cached_attention_fp8 on an fp8 cache against the bf16 kernels on a bf16 cache of the same shape: decode_attention
    at T = 1, chunk_attention at T = 5 / 8; every row's last query sees ``len`` keys.  Both rotate over the same number
    of cache buffers (sized by the bf16 bytes: more than 256 MiB for the fp8 caches too)."""
    lines = [f"{'B':>3s} {'H':>3s} {'Hkv':>3s} {'D':>4s} {'len':>5s} {'T':>2s} {'bf16 us':>9s} {'TB/s':>6s} {'fp8 us':>9s} "
             f"{'TB/s':>6s} {'fp8 / bf16 time':>15s} {'bytes ratio':>11s}"]
    for B, H, Hkv, D, L in KERNEL_SHAPES:
        bytes16 = 2 * B * Hkv * L * D * 2
        bytes8 = 2 * B * Hkv * L * (D + 4)
        n = max(2, min(64, -(-3 * CACHE_BYTES // bytes16)))
        g = torch.Generator(device=dev).manual_seed(0)
        caches = [torch.randn(2, B, L, Hkv, D, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(n)]
        codes = [torch.empty(2, B, L, Hkv, D, device=dev, dtype=torch.uint8) for _ in range(n)]
        scales = [torch.empty(2, B, L, Hkv, device=dev, dtype=torch.float32) for _ in range(n)]
        for c16, c8, s8 in zip(caches, codes, scales):
            for j in range(2):
                fused.kv_quantize(c16[j], c8[j], s8[j])
        for T in chunks:
            q = torch.randn(B, T, H, D, device=dev, dtype=torch.bfloat16, generator=g)
            before = torch.full((B,), L - T, dtype=torch.int32, device=dev)
            full = torch.full((B,), L, dtype=torch.int32, device=dev)
            if T == 1:
                t16 = _time(lambda i: fused.decode_attention(q[:, 0], caches[i][0], caches[i][1], full, 0, L), n, iters)
            else:
                t16 = _time(lambda i: fused.chunk_attention(q, caches[i][0], caches[i][1], before, None, 0, L), n, iters)
            t8 = _time(lambda i: fused.cached_attention_fp8(q, codes[i][0], scales[i][0], codes[i][1], scales[i][1], before,
                                                            None, 0, L), n, iters)
            lines.append(f"{B:3d} {H:3d} {Hkv:3d} {D:4d} {L:5d} {T:2d} {t16 * 1e6:9.1f} {bytes16 / t16 / 1e12:6.2f} "
                         f"{t8 * 1e6:9.1f} {bytes8 / t8 / 1e12:6.2f} {t8 / t16:15.2f} {bytes8 / bytes16:11.2f}")
        del caches, codes, scales
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


# ------------------------------------------------------------------------------------------ LM-head sampling
SAMPLE_HEADS = [("gpt2", 50257, 768), ("llama-3-8b", 128256, 4096)]
SAMPLE_ROWS = (1, 8, 16)
SAMPLE_KW = dict(temperature=0.8, top_k=50, top_p=0.95)


def sample_table(dev, iters):
    """csrc/lm_sample.hip against the chain generate(sampler="torch") runs on the same bf16 logits (warp_logits,
    softmax, multinomial), and fused.lm_head_sample against the head GEMM + that chain.  Device time is the summed
    kernel durations of a profiler trace per call (_device_time), wall time is device events around back-to-back
    calls (_time): the chain is a dozen short launches, so its wall time is what a decode step pays.  The logits
    are 2 * randn in bf16 and rotate over 4 buffers that stay inside the L2 / Infinity Cache, as after the GEMM."""
    from distributed_lion_pytorch_amd.models.generation import warp_logits
    from distributed_lion_pytorch_amd.ops.reference import sr_key

    t, k, p = SAMPLE_KW["temperature"], SAMPLE_KW["top_k"], SAMPLE_KW["top_p"]
    inv_t = torch.tensor(1.0 / t, dtype=torch.float32).item()
    lines = [f"{'head':>10s} {'V':>6s} {'N':>2s} | {'kernel us':>9s} {'chain us':>8s} {'chain/kernel':>12s} | {'kernel wall us':>14s} "
             f"{'chain wall us':>13s} {'ratio':>6s} | {'GEMM+kernel wall us':>19s} {'GEMM+chain wall us':>18s} {'ratio':>6s} | kept"]
    g = torch.Generator(device=dev).manual_seed(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    for name, V, C in SAMPLE_HEADS:
        # a Parameter, as a model's head: its padded copy is cached instead of rebuilt per call
        w = torch.nn.Parameter((torch.randn(V, C, device=dev, generator=g) * 0.02).bfloat16(), requires_grad=False)
        for N in SAMPLE_ROWS:
            vp = (V + 63) // 64 * 64
            xs = [(2 * torch.randn(N, vp, device=dev, generator=g)).bfloat16() for _ in range(4)]
            hs = [torch.randn(N, C, device=dev, generator=g).bfloat16() for _ in range(4)]

            def kernel(i):
                return hip.ops().lm_sample(xs[i], V, inv_t, k, p, sr_key(0, i))

            def chain(i, logits=None):
                x = xs[i][:, :V] if logits is None else logits
                return torch.multinomial(warp_logits(x, t, k, p).softmax(-1), 1, generator=gen)[:, 0]

            with torch.no_grad():
                d_k, d_c = _device_time(kernel, 4, iters), _device_time(chain, 4, iters)
                w_k, w_c = _time(kernel, 4, iters), _time(chain, 4, iters)
                o_k = _time(lambda i: fused.lm_head_sample(hs[i], w, seed=0, step=i, **SAMPLE_KW), 4, iters)
                o_c = _time(lambda i: chain(i, linear.gemm_fwd(hs[i], w)), 4, iters)
            kept = hip.ops().lm_sample(xs[0], V, inv_t, k, p, 0)[3].tolist()
            row = (f"{name:>10s} {V:6d} {N:2d} | {d_k * 1e6:9.1f} {d_c * 1e6:8.1f} {d_c / d_k:11.2f}x | {w_k * 1e6:14.1f} "
                   f"{w_c * 1e6:13.1f} {w_c / w_k:5.2f}x | {o_k * 1e6:19.1f} {o_c * 1e6:18.1f} {o_c / o_k:5.2f}x | "
                   f"{min(kept)}..{max(kept)}")
            lines.append(row)
            print(row, flush=True)
            del xs, hs
        del w
        torch.cuda.empty_cache()
    return lines


def sample_end_to_end(model_name, dev, prompt=128, new=64):
    """A generate decode step with each sampler at B in SAMPLE_ROWS: (wall(new tokens) - wall(1 token)) / (new - 1),
    the two samplers alternating over two rounds, the better round of each reported."""
    cfg = load_config(model_name)
    torch.manual_seed(0)
    with torch.device(dev):
        model = build_model(cfg, native=True).to(dtype=torch.bfloat16)
    model.eval()
    lines = [f"{model_name}: {prompt} prompt + {new} new tokens, bf16, random weights, do_sample=True {SAMPLE_KW}"]
    for B in SAMPLE_ROWS:
        ids = torch.randint(0, cfg.vocab_size, (B, prompt), device=dev)
        per = {"torch": [], "fused": []}
        for sampler in per:
            model.generate(ids, max_new_tokens=4, do_sample=True, seed=0, sampler=sampler, **SAMPLE_KW)  # warm-up
        for _ in range(2):
            for sampler in per:
                def call(n):
                    return model.generate(ids, max_new_tokens=n, do_sample=True, seed=0, sampler=sampler, **SAMPLE_KW)
                tn, _ = _wall(lambda: call(new))
                t1, _ = _wall(lambda: call(1))
                per[sampler].append((tn - t1) / (new - 1) * 1e3)
        a, b = min(per["torch"]), min(per["fused"])
        lines.append(f"  B = {B:2d}: ms per decode step  torch {a:.3f} (rounds {per['torch'][0]:.3f} {per['torch'][1]:.3f})  "
                     f"fused {b:.3f} (rounds {per['fused'][0]:.3f} {per['fused'][1]:.3f})  fused / torch {b / a:.3f}")
        print(lines[-1], flush=True)
    del model
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


SHARED_HEADS = [("gpt2", 12, 12, 64), ("llama-3-8b", 32, 8, 128)]


def beam_shared_table(dev, iters, Bp=2, suffix=64):
    """fused.shared_prefix_attention (one prefix cache row per prompt, csrc/prefix_attention.hip) against
    fused.decode_attention on the repeated cache (one row per beam) at the same prompt / suffix lengths: both over
    distinct caches that sweep 3 x 256 MiB per measurement, alternating, the better of two rounds each."""
    lines = [f"{'heads':>11s} {'Bp':>3s} {'beams':>5s} {'prompt':>6s} {'suffix':>6s} {'S1+S2':>6s} {'repeated us':>11s} "
             f"{'shared us':>10s} {'shared / repeated':>17s} {'max |diff|':>10s}"]
    for name, H, Hkv, D in SHARED_HEADS:
        for nb in (4, 8):
            for L in (2048, 16384):
                rows = Bp * nb
                g = torch.Generator(device=dev).manual_seed(0)

                def variants(row_bytes):
                    return max(2, min(64, -(-3 * CACHE_BYTES // row_bytes)))

                n_s = variants(2 * Bp * Hkv * L * D * 2)
                n_r = variants(2 * rows * Hkv * (L + suffix) * D * 2)
                pre = [torch.randn(2, Bp, L, Hkv, D, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(n_s)]
                suf = torch.randn(2, rows, suffix, Hkv, D, device=dev, dtype=torch.bfloat16, generator=g)
                full = [torch.empty(2, rows, L + suffix, Hkv, D, device=dev, dtype=torch.bfloat16) for _ in range(n_r)]
                for i, c in enumerate(full):  # the repeated cache of prefix variant i: the same keys, nb copies
                    c[:, :, :L] = pre[i % n_s].repeat_interleave(nb, dim=1)
                    c[:, :, L:] = suf
                q = torch.randn(rows, H, D, device=dev, dtype=torch.bfloat16, generator=g)
                plen = torch.full((Bp,), L, dtype=torch.int32, device=dev)
                slen = torch.full((rows,), suffix, dtype=torch.int32, device=dev)
                tlen = torch.full((rows,), L + suffix, dtype=torch.int32, device=dev)

                def shared(i):
                    return fused.shared_prefix_attention(q, pre[i][0], pre[i][1], plen, suf[0], suf[1], slen, nb)

                def repeated(i):
                    return fused.decode_attention(q, full[i][0], full[i][1], tlen, 0, L + suffix)

                err = float((shared(0).float() - repeated(0).float()).abs().max())
                t_s, t_r = [], []
                for _ in range(2):
                    t_r.append(_time(repeated, n_r, iters))
                    t_s.append(_time(shared, n_s, iters))
                (s1, _), (s2, _) = fused.shared_prefix_splits(Bp, nb, Hkv, L, suffix)
                lines.append(f"{name:>11s} {Bp:3d} {nb:5d} {L:6d} {suffix:6d} {s1:3d}+{s2:<2d} {min(t_r) * 1e6:11.1f} "
                             f"{min(t_s) * 1e6:10.1f} {min(t_s) / min(t_r):17.3f} {err:10.1e}")
                del pre, full, suf
                torch.cuda.empty_cache()
    return lines


def beam_end_to_end(name, dev, num_beams, shared=False, prompt=None):
    """Beam search at B / num_beams prompts against greedy at B rows on the same model: the decode kernels and
    the GEMMs see the same M.  ``shared``: also beam search with ``beam_cache="shared"``, alternating with the others."""
    s = dict(E2E[name], **({} if prompt is None else {"prompt": prompt}))
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
        calls = [("greedy", lambda n: model.generate(ids, max_new_tokens=n)),
                 ("beam", lambda n: model.generate(ids[:Bb], max_new_tokens=n, **kw))]
        if shared:
            calls.append(("shared", lambda n: model.generate(ids[:Bb], max_new_tokens=n, beam_cache="shared", **kw)))
        for what, call in calls:
            t, out = _wall(lambda: call(new))
            assert out.shape == (rows, s["prompt"] + new), out.shape
            t1, _ = _wall(lambda: call(1))
            per.setdefault(what, []).append((t - t1) / (new - 1) * 1e3)
            lines.append(f"  round {rnd} {what:6s}: {t:.3f} s, prefill + first token {t1 * 1e3:.1f} ms, "
                         f"{per[what][-1]:.3f} ms per step")
    g, b = min(per["greedy"]), min(per["beam"])
    lines.append(f"  ms per step: beam {b:.3f}, greedy {g:.3f}, beam / greedy {b / g:.3f}")
    if shared:
        lines.append(f"  ms per step: beam on a shared prompt cache {min(per['shared']):.3f}, shared / repeated "
                     f"{min(per['shared']) / b:.3f}")
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
    ap.add_argument("--sample", action="store_true",
                    help="the LM-head sampling kernel (csrc/lm_sample.hip) and fused.lm_head_sample against the warp_logits "
                         "+ multinomial chain, and a generate decode step with each sampler, on GPT-2 and Llama-3-8B")
    ap.add_argument("--num_beams", type=int, default=1,
                    help="end to end: beam search at B / num_beams prompts next to greedy at B rows, instead of the "
                         "generate / naive-loop / phase report")
    ap.add_argument("--kv_cache_dtype", default=None, choices=("fp8_e4m3",),
                    help="the kernel table's fp8 axis: cached_attention_fp8 (csrc/kv8_attention.hip) at T = 1 / 5 / 8 "
                         "against decode_attention / chunk_attention on a bf16 cache of the same shape")
    ap.add_argument("--beam_cache", default="repeated", choices=("repeated", "shared"),
                    help="shared: the shared-prefix attention table (csrc/prefix_attention.hip against decode_attention "
                         "on the repeated cache) and, with --num_beams, beam search end to end both ways")
    ap.add_argument("--e2e_prompt", type=int, default=None, help="with --num_beams: the prompt length, instead of the preset's")
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
    if a.kv_cache_dtype == "fp8_e4m3":
        head = ["## cached_attention_fp8 on an fp8 (e4m3) cache against the bf16 kernels on a bf16 cache, every row at "
                "full length; K+V bytes (codes and scales for fp8) over kernel time", ""]
        print("\n".join(head), flush=True)
        report += head + kv8_table(dev, a.iters) + [""]
        print("\n".join(report[-len(KERNEL_SHAPES) * 3 - 2:]), flush=True)
    if a.beam_cache == "shared":
        head = ["## shared_prefix_attention (csrc/prefix_attention.hip) against decode_attention on the repeated cache, "
                "bf16, every row at full length; back-to-back calls between device events", ""]
        print("\n".join(head), flush=True)
        report += head + beam_shared_table(dev, a.iters) + [""]
        print("\n".join(report[-10:]), flush=True)
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
    if a.sample:
        head = ["## LM-head sampling (csrc/lm_sample.hip) against warp_logits + softmax + multinomial on the same bf16 "
                f"logits, {SAMPLE_KW}; device time = summed kernel durations of a profiler trace, wall = back-to-back calls", ""]
        print("\n".join(head), flush=True)
        report += head + sample_table(dev, a.iters) + ["", "## generate decode step by sampler", ""]
        for name, _, _ in SAMPLE_HEADS:
            report += sample_end_to_end(name, dev) + [""]
    if not a.skip_e2e:
        report += ["## end to end", ""]
        for name in a.e2e or sorted(E2E):
            if a.num_beams > 1:
                lines = beam_end_to_end(name, dev, a.num_beams, a.beam_cache == "shared", a.e2e_prompt)
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
