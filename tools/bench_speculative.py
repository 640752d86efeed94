#!/usr/bin/env python
"""Speculative-decoding benchmarks (needs the GPU).  Writes a text report (default profiles/speculative.txt).

(a) ``fused.chunk_attention`` at T = 5 and T = 8 against T calls of ``fused.decode_attention`` on the same caches
    (B in {1, 8}, context 4096, Llama-3-8B and GPT-2 head geometry, and 32 heads on 4 kv heads): device time and the K/V bytes per second
    each form reaches, the bytes being what one pass over the caches has to read (B Hkv len D 2 bytes, twice).
(b) one cached chunk forward of 6 tokens against one decode step of the same model at B = 1.
(c) ``generate`` tokens/s without an assistant, with the target as its own assistant (nearly every draft accepted: the
    ceiling of the mechanism, at twice the target's cost per round) and with a 1-layer draft of the same geometry
    (random weights: its acceptance says nothing about a trained draft's).

    python tools/bench_speculative.py
    python tools/bench_speculative.py --skip_e2e          # the kernel table only
    python tools/bench_speculative.py --model gpt2        # (b) and (c) on another model

Method as in tools/bench_decode.py: kernel times are the summed kernel durations of a profiler trace, the calls
rotating over enough distinct cache buffers that the working set exceeds the 256 MiB Infinity Cache; end-to-end
figures are wall time around a device synchronise, the better of two alternating rounds."""
from __future__ import annotations

import argparse
import copy
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_decode import CACHE_BYTES, HBM_COPY_TBS, _device_time, _wall, prefill  # noqa: E402
from distributed_lion_pytorch_amd.models.registry import build_model, load_config  # noqa: E402
from distributed_lion_pytorch_amd.ops import fused, hip  # noqa: E402

SHAPES = [(B, 32, 8, 128, 4096) for B in (1, 8)] + [(B, 12, 12, 64, 4096) for B in (1, 8)]
# group size 8 at head_dim 128: 40 and 64 query rows per kv head, the two instantiations that run one block per CU
SHAPES += [(B, 32, 4, 128, 4096) for B in (1, 8)]


def kernel_table(dev, iters):
    lines = [f"{'B':>3s} {'H':>3s} {'Hkv':>3s} {'D':>4s} {'len':>5s} {'T':>2s} {'splits':>6s} {'chunk us':>9s} {'K+V TB/s':>9s} "
             f"{'of copy':>8s} {'decode us':>9s} {'K+V TB/s':>9s} {'T decodes us':>12s} {'chunk / decode':>14s} {'T decodes / chunk':>17s}"]
    for B, H, Hkv, D, L in SHAPES:
        kv_bytes = 2 * B * Hkv * L * D * 2
        n = max(2, min(64, -(-3 * CACHE_BYTES // kv_bytes)))
        g = torch.Generator(device=dev).manual_seed(0)
        caches = [torch.randn(2, B, L + 8, Hkv, D, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(n)]
        kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
        q1 = torch.randn(B, H, D, device=dev, dtype=torch.bfloat16, generator=g)
        t_d = _device_time(lambda i: fused.decode_attention(q1, caches[i][0], caches[i][1], kv_len, 0, L), n, iters)
        for T in (5, 8):
            q = torch.randn(B, T, H, D, device=dev, dtype=torch.bfloat16, generator=g)
            base = kv_len - T  # the chunk's last query sees L keys
            splits, _ = fused.chunk_splits(B, Hkv, L, T)
            t_c = _device_time(lambda i: fused.chunk_attention(q, caches[i][0], caches[i][1], base, None, 0, L), n, iters)
            row = (f"{B:3d} {H:3d} {Hkv:3d} {D:4d} {L:5d} {T:2d} {splits:6d} {t_c * 1e6:9.1f} {kv_bytes / t_c / 1e12:9.2f} "
                   f"{kv_bytes / t_c / 1e12 / HBM_COPY_TBS:8.1%} {t_d * 1e6:9.1f} {kv_bytes / t_d / 1e12:9.2f} {T * t_d * 1e6:12.1f} "
                   f"{t_c / t_d:13.2f}x {T * t_d / t_c:16.2f}x")
            lines.append(row)
            print(row, flush=True)
        del caches
        torch.cuda.empty_cache()
    return lines


@torch.no_grad()
def forward_ratio(model, ids, k=5, reps=20):
    """(seconds per decode step, seconds per chunk forward of k + 1 tokens), the cache rolled back after each."""
    cache, _ = prefill(model, ids, 2 * (k + 1) + 2)
    base = model._decoder()
    lens = cache.lengths.clone()
    width = cache.width
    tok = ids[:, :k + 1].contiguous()

    def step():
        for _ in range(reps):
            base(tok[:, :1], cache=cache)
            cache.truncate(lens, width)

    def chunk():
        for _ in range(reps):
            base(tok, cache=cache)
            cache.truncate(lens, width)

    step(), chunk()  # warm-up
    best = {}
    for _ in range(2):
        for name, fn in (("step", step), ("chunk", chunk)):
            t, _ = _wall(fn)
            best[name] = min(best.get(name, t), t)
    return best["step"] / reps, best["chunk"] / reps


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
    lines = [f"{name}: B = {B}, {prompt} prompt + {new} new tokens, bf16, random weights, greedy, num_assistant_tokens = {k}"]
    t_s, t_c = forward_ratio(model, ids, k)
    lines.append(f"  (b) one decode step {t_s * 1e3:.3f} ms, one chunk forward of {k + 1} tokens {t_c * 1e3:.3f} ms: "
                 f"ratio {t_c / t_s:.2f} (all {k} drafts accepted: {(k + 1) * t_s / t_c:.2f}x fewer target ms per token)")
    runs = {"plain": dict(), "self-draft (the target as its own assistant)": dict(assistant_model=model, num_assistant_tokens=k),
            "1-layer random draft (acceptance meaningless)": dict(assistant_model=draft, num_assistant_tokens=k)}
    for kw in runs.values():
        model.generate(ids, max_new_tokens=2 * k + 3, **kw)  # warm-up: code objects, GEMM algorithm choices
    best, info = {}, {}
    for _ in range(2):
        for what, kw in runs.items():
            t, out = _wall(lambda: model.generate(ids, max_new_tokens=new, return_dict_in_generate=True, **kw))
            t1, _ = _wall(lambda: model.generate(ids, max_new_tokens=1, **kw))
            best[what] = min(best.get(what, t - t1), t - t1)
            if kw:
                info[what] = f"; {out.rounds} rounds, accepted per row {out.accepted.tolist()} of {new - 1}"
    for what in runs:
        lines.append(f"  (c) {what}: {B * (new - 1) / best[what]:.1f} tokens/s after the first token "
                     f"({best[what] / (new - 1) * 1e3:.3f} ms per token; {best['plain'] / best[what]:.2f}x plain){info.get(what, '')}")
    del model, draft
    torch.cuda.empty_cache()
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "speculative.txt"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--skip_kernel", action="store_true")
    ap.add_argument("--skip_e2e", action="store_true")
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--num_assistant_tokens", type=int, default=5)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_speculative.py measures on the GPU; there is none here")
    hip.require()
    dev = torch.device("cuda", 0)
    report = [f"# tools/bench_speculative.py on {torch.cuda.get_device_name(0)}", ""]
    if not a.skip_kernel:
        report += ["## (a) chunk_attention against decode_attention, bf16, context 4096; K+V bytes of one pass over device "
                   f"time against the {HBM_COPY_TBS} TB/s float4 copy", ""] + kernel_table(dev, a.iters) + [""]
    if not a.skip_e2e:
        lines = end_to_end(a.model, dev, a.batch, a.prompt, a.new, a.num_assistant_tokens)
        print("\n".join(lines), flush=True)
        report += ["## (b), (c) cached forwards and generate", ""] + lines + [""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(report))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
