"""Inputs, fp64 / fp32 forms and bounds shared by tests/test_qk_norm_cpu.py and
tests/test_qk_norm_gpu.py (the per-head q/k RMSNorm + RoPE op, csrc/qk_norm.hip).

Everything is drawn on the host from a seeded generator, so that the CPU and
the GPU tests see the same data.  The reference is fused.qk_norm_rope_reference
(HF's Qwen3RMSNorm order, then the rotate-half rotation) evaluated in fp64; the
allowance for evaluating it in fp32 is EVAL_MARGIN x the error of the same form
in fp32 (numerics.eval_floor's construction, one value per head row)."""
import torch

import numerics as nm
from distributed_lion_pytorch_amd.ops import fused

EPS = 1e-6
B = 2
SHAPES = [(T, H, Hkv, D) for D in (128, 64) for T in (1, 33, 100) for (H, Hkv) in ((4, 2), (2, 2), (3, 1))]


def inputs(T, H, Hkv, D, seed=0):
    """x [B, T, H + Hkv, D] bf16 (q heads then k heads), dz of the same shape,
    gamma_q / gamma_k [D], cos / sin [T + 5, D]: independent, asymmetric tables
    uniform in (-1, 1) -- no true rotation, so a swapped half or partner shows.
    Rows: one all-zero head row (r = eps^-1/2), one token scaled by 2^20, one by
    2^-20, one row with a single non-zero element."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * T + 3 * H + Hkv + D)
    Hx = H + Hkv
    x = torch.randn(B, T, Hx, D, generator=g)
    x[1, 0] *= 2.0 ** 20
    x[0, T - 1] *= 2.0 ** -20
    x[0, 0, 0] = 0.0
    x[1, T // 2, Hx - 1] = 0.0
    x[1, T // 2, Hx - 1, 5] = 1.5
    dz = torch.randn(B, T, Hx, D, generator=g)
    gq = 1.0 + 0.25 * torch.randn(D, generator=g)
    gk = 1.0 + 0.25 * torch.randn(D, generator=g)
    gq[3], gq[D // 2 + 7] = 0.0, -gq[D // 2 + 7].abs()
    gk[D // 2 + 2], gk[9] = 0.0, -gk[9].abs()
    cos = torch.rand(T + 5, D, generator=g) * 2 - 1
    sin = torch.rand(T + 5, D, generator=g) * 2 - 1
    return tuple(t.to(torch.bfloat16) for t in (x, dz, gq, gk, cos, sin))


def identity_tables(T, D, like):
    """cos = 1, sin = 0: the rotation is the identity, exactly (x 1 + rot 0)."""
    return torch.ones(T, D, dtype=like.dtype, device=like.device), torch.zeros(T, D, dtype=like.dtype, device=like.device)


def form(x, gq, gk, split, cos, sin, dz, dtype, rotate=True):
    """The PyTorch form in ``dtype`` (fp32 or fp64) on the CPU: (z, dx, dgq, dgk)
    with dx / dgamma from autograd for the output gradient dz.  ``rotate`` False:
    no rotation (dz is then the gradient of gamma x-hat itself)."""
    x, gq, gk, cos, sin, dz = (t.detach().cpu().to(dtype) for t in (x, gq, gk, cos, sin, dz))
    if not rotate:
        cos, sin = identity_tables(x.shape[1], x.shape[-1], x)
    x.requires_grad_()
    gq.requires_grad_()
    gk.requires_grad_()
    z = torch.cat([fused.qk_norm_rope_reference(x[:, :, :split], gq, EPS, cos, sin),
                   fused.qk_norm_rope_reference(x[:, :, split:], gk, EPS, cos, sin)], 2)
    z.backward(dz)
    return z.detach(), x.grad, gq.grad, gk.grad


def row_floor(f32: torch.Tensor, f64: torch.Tensor) -> torch.Tensor:
    """[B, T, Hx, 1] fp64: EVAL_MARGIN x the head row's largest |fp32 form - fp64 form|."""
    return nm.EVAL_MARGIN * (f32.double() - f64).abs().amax(-1, keepdim=True)


def stats64(x):
    """(x-hat, rstd) in fp64: x [B, T, Hx, D] -> [B, T, Hx, D], [B, T, Hx]."""
    x64 = x.detach().cpu().double()
    r = torch.rsqrt(x64.pow(2).mean(-1) + EPS)
    return x64 * r[..., None], r


def part_ranges(rows, parts):
    """Token-row range of each partial row: part p owns [p rpp, min((p + 1) rpp, rows)), rpp = ceil(rows / parts)."""
    rpp = (rows + parts - 1) // parts
    return [(min(p * rpp, rows), min((p + 1) * rpp, rows)) for p in range(parts)]


def assert_gain_partials(part, x, dz, cos, sin, split, parts, floor_fwd, rotate, name=""):
    """part [parts, 2, D] fp32 against the fp64 sums of dy x-hat over each part's own token rows, q heads
    (< split) and k heads apart, x-hat from the fp64 reference.  With ``rotate`` dy = rope^T(dz) is itself the
    sum of two products, dz cos and its partner's dz sin, so each row contributes two terms to a column; without,
    dy = dz and it contributes one.  Bound per part and column: n 2^-24 sum |terms| (an fp32 sum of the n terms
    in any order) + sum over the rows of the row's forward floor x |dy| (x-hat evaluated in fp32).  A part
    without rows is exactly zero.  Prints and returns the largest err / bound."""
    Bn, T, Hx, D = x.shape
    xh, _ = stats64(x)
    dz64 = dz.detach().cpu().double()
    if rotate:
        c, s = cos.detach().cpu().double()[None, :T, None, :], sin.detach().cpu().double()[None, :T, None, :]
        d2 = D // 2
        z = dz64 * s
        zp = torch.cat([z[..., d2:], -z[..., :d2]], -1)
        dy, mag, per_row = dz64 * c + zp, ((dz64 * c).abs() + zp.abs()) * xh.abs(), 2
    else:
        dy, mag, per_row = dz64, (dz64 * xh).abs(), 1
    terms = (dy * xh).reshape(Bn * T, Hx, D)
    mag = mag.reshape(Bn * T, Hx, D)
    slack = (floor_fwd.double() * dy.abs()).reshape(Bn * T, Hx, D)
    got = part.detach().cpu().double()
    assert part.dtype == torch.float32 and tuple(part.shape) == (parts, 2, D), (part.dtype, tuple(part.shape))
    assert torch.isfinite(got).all(), f"{name}: non-finite partials"
    worst = 0.0
    for p, (r0, r1) in enumerate(part_ranges(Bn * T, parts)):
        for blk, hs in enumerate((slice(0, split), slice(split, Hx))):
            n = per_row * (r1 - r0) * len(range(*hs.indices(Hx)))
            if n == 0:
                assert bool((part[p, blk] == 0).all()), f"{name}: part {p} block {blk} has no rows but is not zero"
                continue
            ref = terms[r0:r1, hs].sum((0, 1))
            bound = n * nm.SUM_EPS * mag[r0:r1, hs].sum((0, 1)) + slack[r0:r1, hs].sum((0, 1))
            err = (got[p, blk] - ref).abs()
            ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
            worst = max(worst, float(ratio.max()))
            if not bool((err <= bound).all()):
                j = int(torch.argmax(ratio))
                raise AssertionError(f"{name}: part {p} block {blk} column {j}: got {float(got[p, blk, j]):.9e} "
                                     f"ref {float(ref[j]):.9e} bound {float(bound[j]):.3e}")
    print(f"[gain partials] {name}: max err / bound {worst:.3f}")
    return worst


def emulate_fwd32(x, gq, gk, split, cos, sin):
    """A second fp32 realisation of the forward with another summation order
    (pairs inside groups of 8, then a butterfly over the groups) and the
    rotation written per half: what a lane-per-8-dims kernel computes."""
    x, gq, gk, cos, sin = (t.detach().cpu().float() for t in (x, gq, gk, cos, sin))
    Bn, T, Hx, D = x.shape
    sq = (x * x).reshape(Bn, T, Hx, D // 8, 8)
    s = ((sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3])) + ((sq[..., 4] + sq[..., 5]) + (sq[..., 6] + sq[..., 7]))
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    r = 1.0 / torch.sqrt(s * (1.0 / D) + torch.tensor(EPS, dtype=torch.float32))
    gam = torch.cat([gq.expand(split, D), gk.expand(Hx - split, D)], 0)
    y = (x * r) * gam
    d2 = D // 2
    c, sn = cos[None, :T, None, :], sin[None, :T, None, :]
    lo = y[..., :d2] * c[..., :d2] - y[..., d2:] * sn[..., :d2]
    hi = y[..., d2:] * c[..., d2:] + y[..., :d2] * sn[..., d2:]
    return torch.cat([lo, hi], -1), r.squeeze(-1)
