#!/usr/bin/env python
"""Speculative-sampling benchmarks (needs the GPU).  Writes a text report (default profiles/spec_sample.txt).

(a) the verify kernel (``fused.speculative_verify``, csrc/spec_verify.hip) against its PyTorch form
    (``fused._spec_verify_torch``) on the same GPU tensors: bf16 logits, kk = 5 drafts, V in {50257, 128256},
    B in {1, 8, 16}, unfiltered and under (temperature 0.8, top-k 50, top-p 0.95); draft logits are the target's plus
    unit noise, so a good part of the positions is rejected and takes the kernel's second sweep.
(b) ``generate(do_sample=True)`` per emitted token: ``sampler="fused"`` against ``sampler="speculative"`` with the
    target as its own assistant (q is p up to the cached paths' rounding: the mechanism's ceiling at twice the target's
    cost per round) and with a 1-layer draft of the same geometry (random weights: its acceptance says nothing about
    a trained draft's).

    python tools/bench_spec_sample.py
    python tools/bench_spec_sample.py --skip_e2e          # the kernel table only
    python tools/bench_spec_sample.py --model gpt2        # (b) on another model

Method as in tools/bench_decode.py: kernel times are the summed kernel durations of a profiler trace, the calls
rotating over distinct input sets (enough to exceed the 256 MiB Infinity Cache where 16 sets can; the small shapes stay
cache-resident, as they are behind the head GEMM that has just written them); end-to-end figures are wall time around
a device synchronise, the better of two alternating rounds."""
from __future__ import annotations

import argparse
import copy
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_decode import CACHE_BYTES, _device_time, _wall  # noqa: E402
from distributed_lion_pytorch_amd.models.registry import build_model, load_config  # noqa: E402
from distributed_lion_pytorch_amd.ops import fused, hip  # noqa: E402

KK = 5
SETTINGS = ((1.0, 0, 1.0), (0.8, 50, 0.95))


def kernel_table(dev, iters):
    lines = [f"{'V':>7s} {'B':>3s} {'kk':>2s} {'temp':>5s} {'top_k':>5s} {'top_p':>5s} {'sets':>4s} {'rejected':>8s} "
             f"{'kernel us':>10s} {'logit GB/s':>10s} {'torch-form us':>13s} {'speedup':>8s}"]
    for v in (50257, 128256):
        vp = (v + 63) // 64 * 64
        for B in (1, 8, 16):
            nbytes = B * (2 * KK + 1) * vp * 2
            n = max(2, min(16, -(-2 * CACHE_BYTES // nbytes)))
            g = torch.Generator(device=dev).manual_seed(v + B)
            for t, top_k, top_p in SETTINGS:
                sets = []
                for _ in range(n):
                    T = (4 * torch.randn(B, KK + 1, vp, device=dev, generator=g)).bfloat16()
                    D = (T[:, :KK].float() + torch.randn(B, KK, vp, device=dev, generator=g)).bfloat16()
                    d = fused.lm_sample(D.view(-1, vp), v, t, top_k, top_p, seed=1, step=0)
                    tt = fused.lm_sample(T.view(-1, vp), v, t, top_k, top_p, seed=1, step=1)
                    sets.append((T, D, d.ids.view(B, KK), tt.floor.view(B, KK + 1), d.floor.view(B, KK),
                                 tt.ids.view(B, KK + 1)[:, KK].contiguous()))
                rejected = sum(float(1 - fused.speculative_verify(*s, v, t, 1, 2).flags.float().mean()) for s in sets) / n
                t_k = _device_time(lambda i: fused.speculative_verify(*sets[i], v, t, 1, 2), n, iters)
                fused.set_impl("torch")
                try:
                    t_t = _device_time(lambda i: fused.speculative_verify(*sets[i], v, t, 1, 2), n, max(2, iters // 10))
                finally:
                    fused.set_impl("auto")
                row = (f"{v:7d} {B:3d} {KK:2d} {t:5.2f} {top_k:5d} {top_p:5.2f} {n:4d} {rejected:8.1%} {t_k * 1e6:10.1f} "
                       f"{nbytes / t_k / 1e9:10.1f} {t_t * 1e6:13.1f} {t_t / t_k:7.1f}x")
                lines.append(row)
                print(row, flush=True)
                del sets
            torch.cuda.empty_cache()
    return lines


def end_to_end(name, dev, B, prompt, new, k):
    cfg = load_config(name)
    torch.manual_seed(0)
    with torch.device(dev):
        model = build_model(cfg, native=True).to(dtype=torch.bfloat16)
        dcfg = copy.deepcopy(cfg)
        if hasattr(dcfg, "num_hidden_layers"):
            dcfg.num_hidden_layers = 1
            if getattr(dcfg, "layer_types", None):
                dcfg.layer_types = dcfg.layer_types[:1]
        else:
            dcfg.n_layer = 1
        draft = build_model(dcfg, native=True).to(dtype=torch.bfloat16)
    model.eval(), draft.eval()
    ids = torch.randint(0, cfg.vocab_size, (B, prompt), device=dev)
    warp = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.95, seed=0)
    lines = [f"{name}: B = {B}, {prompt} prompt + {new} new tokens, bf16, random weights, temperature 0.8, top-k 50, "
             f"top-p 0.95, num_assistant_tokens = {k}"]
    spec = dict(sampler="speculative", num_assistant_tokens=k)
    runs = {"sampler='fused'": dict(sampler="fused"),
            "speculative, self-draft (the target as its own assistant)": dict(assistant_model=model, **spec),
            "speculative, 1-layer random draft (acceptance meaningless)": dict(assistant_model=draft, **spec)}
    for kw in runs.values():
        model.generate(ids, max_new_tokens=2 * k + 3, **warp, **kw)  # warm-up: code objects, GEMM algorithm choices
    best, info = {}, {}
    for _ in range(2):
        for what, kw in runs.items():
            t, out = _wall(lambda: model.generate(ids, max_new_tokens=new, return_dict_in_generate=True, **warp, **kw))
            t1, _ = _wall(lambda: model.generate(ids, max_new_tokens=1, **warp, **kw))
            best[what] = min(best.get(what, t - t1), t - t1)
            if "assistant_model" in kw:
                info[what] = f"; {out.rounds} rounds, accepted drafts per row {out.accepted.tolist()} of {new - 1} tokens"
    ref = best["sampler='fused'"]
    for what in runs:
        lines.append(f"  {what}: {B * (new - 1) / best[what]:.1f} tokens/s after the first token "
                     f"({best[what] / (new - 1) * 1e3:.3f} ms per token; {ref / best[what]:.2f}x fused){info.get(what, '')}")
    del model, draft
    torch.cuda.empty_cache()
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "spec_sample.txt"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--skip_kernel", action="store_true")
    ap.add_argument("--skip_e2e", action="store_true")
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--num_assistant_tokens", type=int, default=KK)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_spec_sample.py measures on the GPU; there is none here")
    hip.require()
    dev = torch.device("cuda", 0)
    report = [f"# tools/bench_spec_sample.py on {torch.cuda.get_device_name(0)}", ""]
    if not a.skip_kernel:
        report += ["## (a) the verify kernel against its PyTorch form on the GPU, bf16 logits; logit GB/s = the bytes of "
                   "both blocks once over the kernel's device time", ""] + kernel_table(dev, a.iters) + [""]
    if not a.skip_e2e:
        lines = end_to_end(a.model, dev, a.batch, a.prompt, a.new, a.num_assistant_tokens)
        print("\n".join(lines), flush=True)
        report += ["## (b) generate per emitted token", ""] + lines + [""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(report))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
