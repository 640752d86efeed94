"""Lion optimizer kernels against the HBM roofline (one MI355X, bf16 params):
K0 local update, K1 encode (momentum + 1-bit pack), K2 vote+apply over W
fake voter planes, K4 shard vote (a2a), the average vote's byte kernel against
its a2a path (K4c shard count + counted apply), over the GPT-2 small and the
Llama-3-8B parameter sets (shapes only, random values).  Bytes per param are
the kernels' compulsory traffic; prints us (median, min-max over the rounds),
GB/s and % of 6.3 TB/s.

  python tools/bench_lion.py [gpt2|llama3] [W] [--param_rounding nearest|stochastic|both]

``--param_rounding both`` times K0 and the pre-voted K2 with the nearest and
the stochastic parameter store interleaved in one process (the cost of the
coordinate hash); ``--only_rounding`` keeps just those cases.  With
``DLION_LIB`` naming an earlier build of the extension, use ``nearest``.
"""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, ".")
from distributed_lion_pytorch_amd.ops import hip  # noqa: E402
from distributed_lion_pytorch_amd.ops import reference as ref  # noqa: E402
from distributed_lion_pytorch_amd.optim.executors import HParams, HipExecutor  # noqa: E402
from distributed_lion_pytorch_amd.optim.plan import FlatPlan  # noqa: E402

HBM = 6.3e12


def shapes(model):
    if model == "gpt2":
        C, L, V = 768, 12, 50257
        per = [(3 * C, C), (3 * C,), (C, C), (C,), (4 * C, C), (4 * C,), (C, 4 * C), (C,), (C,), (C,), (C,), (C,)]
        return [(V, C), (1024, C)] + per * L + [(C,), (C,)]
    C, L, V, F, KV = 4096, 32, 128256, 14336, 1024
    per = [(C, C), (KV, C), (KV, C), (C, C), (F, C), (F, C), (C, F), (C,), (C,)]
    return [(V, C)] + per * L + [(C,), (V, C)]


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", nargs="?", default="gpt2", choices=["gpt2", "llama3"])
    ap.add_argument("W", nargs="?", type=int, default=8)
    ap.add_argument("--param_rounding", default="nearest", choices=["nearest", "stochastic", "both"])
    ap.add_argument("--only_rounding", action="store_true", help="only K0, the pre-voted K2 and the copy")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    model, W = a.model, a.W
    sr = dict(rounding=ref.ROUND_STOCHASTIC, seed=1, step=1)
    base_kw = sr if a.param_rounding == "stochastic" else {}
    dev = torch.device("cuda")
    ps = [torch.randn(s, device=dev, dtype=torch.bfloat16) for s in shapes(model)]
    gs = [torch.randn_like(p) for p in ps]
    ms = [torch.randn_like(p) * 0.1 for p in ps]
    n = sum(p.numel() for p in ps)
    plan = FlatPlan([(p, 0) for p in ps], world=W, device=dev)
    hx = HipExecutor(plan)
    meta = plan.meta(gs, ms)
    hp = HParams(lr=1e-5, wd=0.1, beta1=0.9, beta2=0.99)
    bits = torch.zeros(plan.total_bytes, dtype=torch.uint8, device=dev)
    planes = torch.randint(0, 256, (W * plan.total_bytes,), dtype=torch.uint8, device=dev)
    alive = torch.ones(W, dtype=torch.uint8, device=dev)
    voted = torch.zeros(plan.total_bytes // W, dtype=torch.uint8, device=dev)

    def local():
        for b in plan.buckets:
            hx.local(meta, b, hp, **base_kw)

    def local_sr():
        for b in plan.buckets:
            hx.local(meta, b, hp, **sr)

    def encode():
        for b in plan.buckets:
            hx.encode(meta, b, bits[b.byte_off:b.byte_off + b.nbytes], hp)

    def apply():
        for b in plan.buckets:
            pl = planes[W * b.byte_off: W * (b.byte_off + b.nbytes)]
            hx.apply(meta, b, pl, b.nbytes, alive, ref.VOTE_MAJORITY, ref.TIE_NEGATIVE, None, hp, **base_kw)

    def apply_prevoted():  # a2a (default exchange): one voted plane after the shard vote + all-gather
        for b in plan.buckets:
            hx.apply(meta, b, planes[b.byte_off: b.byte_off + b.nbytes], b.nbytes, alive, ref.VOTE_PREVOTED,
                     ref.TIE_NEGATIVE, None, hp, **base_kw)

    def apply_prevoted_sr():
        for b in plan.buckets:
            hx.apply(meta, b, planes[b.byte_off: b.byte_off + b.nbytes], b.nbytes, alive, ref.VOTE_PREVOTED,
                     ref.TIE_NEGATIVE, None, hp, **sr)

    def vote_reduce():  # a2a: this rank's shard of every bucket, W planes of it
        for b in plan.buckets:
            sh = b.nbytes // W
            hx.vote_reduce(planes[W * b.byte_off: W * b.byte_off + W * sh], sh, alive, ref.TIE_NEGATIVE,
                           voted[b.byte_off // W: b.byte_off // W + sh], None)

    # average vote: the byte kernel over the W gathered planes (all-gather exchange) against the
    # a2a path's K4c shard count + counted apply from the [W][P][shard] count planes (W <= 15)
    P = W.bit_length()
    counted = W <= 15 and not a.only_rounding
    if counted:
        shard_counts = torch.zeros(P * plan.total_bytes // W, dtype=torch.uint8, device=dev)
        counts = torch.zeros(P * plan.total_bytes, dtype=torch.uint8, device=dev)
        for b in plan.buckets:  # true counts of the same planes, shard by shard
            sh = b.nbytes // W
            pl = planes[W * b.byte_off: W * (b.byte_off + b.nbytes)].view(W, b.nbytes)
            for r in range(W):
                o = P * b.byte_off + r * P * sh
                hx.vote_count(pl[:, r * sh:(r + 1) * sh].contiguous().view(-1), sh, alive, counts[o:o + P * sh])

    def apply_average():
        for b in plan.buckets:
            pl = planes[W * b.byte_off: W * (b.byte_off + b.nbytes)]
            hx.apply(meta, b, pl, b.nbytes, alive, ref.VOTE_AVERAGE, ref.TIE_NEGATIVE, None, hp, **base_kw)

    def apply_counted():
        for b in plan.buckets:
            hx.apply(meta, b, counts[P * b.byte_off: P * (b.byte_off + b.nbytes)], b.nbytes // W, alive,
                     ref.VOTE_COUNTED, ref.TIE_NEGATIVE, None, hp, **base_kw)

    def vote_count():  # a2a + average: this rank's shard of every bucket, W planes in, P count planes out
        for b in plan.buckets:
            sh = b.nbytes // W
            o = P * b.byte_off // W
            hx.vote_count(planes[W * b.byte_off: W * b.byte_off + W * sh], sh, alive, shard_counts[o:o + P * sh])

    src = torch.empty(n, dtype=torch.bfloat16, device=dev)
    dst = torch.empty_like(src)

    def copy():  # practical roofline of a 50/50 read/write stream (what K2's p traffic is)
        dst.copy_(src)

    # compulsory bytes per param: p r+w, g r, m r+w (local); g r, m r+w, 1 bit (encode);
    # p r+w + W bits (apply); W bits read + 1 bit written per shard param (vote_reduce, 1/W of params)
    cases = {"K0 local": (local, 10.0), "K1 encode": (encode, 6.0 + 1 / 8),
             f"K2 vote+apply W={W}": (apply, 4.0 + W / 8), "K2 prevoted apply": (apply_prevoted, 4.0 + 1 / 8), f"K4 shard vote W={W}": (vote_reduce, (W + 1) / 8 / W),
             "bf16 copy (reference)": (copy, 4.0)}
    cases[f"K2 average (byte kernel) W={W}"] = (apply_average, 4.0 + W / 8)
    if a.only_rounding:
        cases = {k: v for k, v in cases.items() if k in ("K0 local", "K2 prevoted apply", "bf16 copy (reference)")}
    if a.param_rounding == "both":  # beside their nearest twins: the rounds interleave them
        twins = {"K0 local": ("K0 local (stochastic)", local_sr),
                 "K2 prevoted apply": ("K2 prevoted apply (stochastic)", apply_prevoted_sr)}
        cases = {kk: vv for k, v in cases.items()
                 for kk, vv in ([(k, v)] + ([(twins[k][0], (twins[k][1], v[1]))] if k in twins else []))}
    if counted:
        cases[f"K2 counted apply W={W}"] = (apply_counted, 4.0 + P / 8)
        cases[f"K4c shard count W={W}"] = (vote_count, (W + P) / 8 / W)
    print(f"{model}: {n / 1e6:.1f}M params, {len(ps)} tensors, {len(plan.buckets)} buckets, "
          f"param_rounding={a.param_rounding}, lib={hip.LIB_PATH.name}", flush=True)
    res = {k: [] for k in cases}
    for _ in range(a.rounds):
        for k, (f, _) in cases.items():
            res[k].append(timed(f))
    for k, (f, bpp) in cases.items():
        us = statistics.median(res[k])
        gbs = bpp * n / us / 1e3
        print(f"  {k:32s} {us:9.1f} us ({min(res[k]):.1f}-{max(res[k]):.1f})  {gbs:7.0f} GB/s  "
              f"{100 * gbs * 1e9 / HBM:5.1f}% of 6.3 TB/s", flush=True)


if __name__ == "__main__":
    main()
