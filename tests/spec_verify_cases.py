"""Shared by the speculative-sampling tests: the cases, the fp64 form of csrc/spec_verify.hip's contract taken from the
same fp32 scaled logits, and the conditions any implementation's (accepted, next, flags, resid, px, qx) must meet.

Bounds, with eps = 2^-24 (fp32 round to nearest), C = ceil(v / 4096) chunks of 8 per thread and D = M - (the least
surviving s) of the row.  Every addend exp(s_j - M) of Z reaches the sum through one subtraction and one expf of its
own (2 eps; the subtraction's error sits in the argument), at most 8 C additions and C rescalings (a multiply and
an expf: 3 eps each) in its thread, the rescaling to the wave maximum (3), 6 additions of the wave sum, the
rescaling to the block maximum (3) and at most 8 additions there: 11 C + 22 roundings.  All exponents on that way
are negative and add up to s_j - M, each off by at most eps times itself, so they cost another D eps.  Addends are
positive, hence |Z' - Z| <= tau Z with tau = (11 C + 22 + D) eps -- the mass bound, here relative.  p_x adds a
subtraction in the exponent (within D eps), an expf (2 eps) and a division (eps): rho = tau + (D + 3) eps; sweep 2
multiplies by a rounded reciprocal instead (one eps more) and subtracts (eps of the result): delta_j = (rho_p + eps)
p_j + (rho_q + eps) q_j + eps |w_j|.  The accept test itself is exact on the fp32 p_x and q_x, so a row is decided when
|u - p_x / q_x| > (rho_p + rho_q) p_x / q_x.  A residual score log(w) + g is within lm_sample_cases' Gumbel-score bound
8 eps (|log w| + 32) of the fp64 one.  Second-order terms: every bound is taken 1.001 times (n eps < 1e-3 throughout).
"""
import functools
import math

import torch

from distributed_lion_pytorch_amd.ops import fused
from distributed_lion_pytorch_amd.ops.reference import _M32, _mix32, sr_key

VOCABS = (5, 13, 4099, 16389)
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
SETTINGS = ((1.0, 0, 1.0), (0.7, 7, 1.0), (1.0, 0, 0.9), (0.8, 50, 0.95))  # (temperature, top_k, top_p)
SHAPES = ((1, 1), (3, 4), (2, 7))  # (B, kk)
SAME = (4099, torch.bfloat16, SETTINGS[3], SHAPES[1], True)  # d_logits == t_logits: all accepted, next == bonus
KEY_D, KEY_T, KEY = sr_key(11, 0), sr_key(11, 1), sr_key(11, 2)
EPS, SLACK = 2.0 ** -24, 1.001


@functools.lru_cache(maxsize=None)
def case(v, dtype, setting, shape, same=False):
    """(inputs of the op, fp64 reference) of one case, computed once and left unchanged."""
    t, top_k, top_p = setting
    B, kk = shape
    vp = (v + 63) // 64 * 64
    g = torch.Generator().manual_seed(1000003 * v + 101 * B + kk)
    T = 4 * torch.randn(B, kk + 1, vp, generator=g)
    D = T[:, :kk] + (0 if same else torch.randn(B, kk, vp, generator=g))
    T[0, 0, 1], D[0, 0, 2], T[0, 0, 3] = float("-inf"), float("nan"), float("nan")  # the row with NaN / -inf columns
    for blk in (T, D):
        blk[..., v:] = 3e4
        blk[..., v + 1::2] = float("nan")
    out_col = v - 1  # position (B - 1, kk - 1): the draft is a column the target has removed
    if not same:
        T[B - 1, kk - 1, out_col], D[B - 1, kk - 1, out_col] = float("-inf"), 20.0  # q keeps it under any setting
    T, D = T.to(dtype), D.to(dtype)
    if same:
        D = T[:, :kk].clone()
    inv_t = torch.tensor(1.0 / t, dtype=torch.float32).item()
    d = fused._lm_sample_torch(D.view(-1, vp), v, inv_t, top_k, top_p, KEY_D)
    tt = fused._lm_sample_torch(T.view(-1, vp), v, inv_t, top_k, top_p, KEY_T)
    drafts = d[0].view(B, kk).clone()
    if not same:
        drafts[B - 1, kk - 1] = out_col
    args = (T, D, drafts, tt[2].view(B, kk + 1), d[2].view(B, kk), tt[0].view(B, kk + 1)[:, kk].clone(), v, inv_t, KEY)
    return args, reference(*args)


def _softmax64(x, floor, v, inv_t):
    s = (x[..., :v].float() * torch.tensor(inv_t, dtype=torch.float32)).double()
    alive = torch.isfinite(s) & (s >= floor.double()[..., None])
    s = torch.where(alive, s, torch.full_like(s, float("-inf")))
    p = torch.where(alive, (s - s.max(-1, keepdim=True).values).exp(), torch.zeros_like(s))
    p = p / p.sum(-1, keepdim=True)
    spread = (s.max(-1).values - torch.where(alive, s, torch.full_like(s, float("inf"))).min(-1).values)
    tau = (11 * math.ceil(v / 4096) + 22 + spread) * EPS
    return p, tau + (spread + 3) * EPS  # the probabilities, rho per row


def reference(T, D, drafts, t_floor, d_floor, bonus, v, inv_t, key):
    """fp64: p_x, q_x, their bounds, u, the flags, the ratio margin's excess over its bound, and per row the lower /
    upper bounded residual scores."""
    B, kk = drafts.shape
    p, rho_p = _softmax64(T[:, :kk], t_floor[:, :kk], v, inv_t)
    q, rho_q = _softmax64(D, d_floor, v, inv_t)
    x = drafts.long()[..., None]
    px, qx = p.gather(-1, x)[..., 0], q.gather(-1, x)[..., 0]
    rows = torch.arange(B * kk).view(B, kk)
    u = fused.sample_uniform(rows, key)
    ratio = px / qx
    excess = (u - ratio).abs() - SLACK * (rho_p + rho_q) * ratio
    w = p - q
    delta = SLACK * ((rho_p + EPS)[..., None] * p + (rho_q + EPS)[..., None] * q + EPS * w.abs())
    n = _mix32((_mix32((torch.arange(v) ^ key) & _M32) + rows[..., None] * 0x9E3779B1 + 0x85EBCA6B) & _M32) >> 8
    gum = -torch.log(-torch.log((n.double() + 0.5) * 2.0 ** -24))
    lo_w, hi_w = (w - delta).clamp_min(0), (w + delta).clamp_min(0)
    slack = SLACK * 8 * EPS * (torch.log(lo_w.clamp_min(2.0 ** -149)).abs() + 32)
    lower = torch.where(lo_w > 0, torch.log(lo_w) + gum - slack, torch.full_like(w, float("-inf")))
    upper = torch.where(hi_w > 0, torch.log(hi_w) + gum + slack, torch.full_like(w, float("-inf")))
    return dict(px=px, qx=qx, bound_p=SLACK * rho_p * px, bound_q=SLACK * rho_q * qx, flags=u * qx < px, excess=excess,
                may=upper >= lower.max(-1, keepdim=True).values)


def check(out, args, ref, name, same=False):
    """The conditions on an implementation's outputs and, first, the two conditions on the case itself."""
    accepted, nxt, flags, resid, px, qx = (o.cpu() for o in out)
    bonus, kk = args[5], args[2].shape[1]
    assert bool((ref["excess"] > 0).all()), f"{name}: an accept test is not decided, excess {ref['excess'].min()}"
    rejected = ~ref["flags"]
    assert bool((ref["may"].sum(-1)[rejected] == 1).all()), f"{name}: a residual draw is not decided"
    assert bool(((px.double() - ref["px"]).abs() <= ref["bound_p"] + 1e-44).all()), f"{name}: px outside its bound"
    assert bool(((qx.double() - ref["qx"]).abs() <= ref["bound_q"] + 1e-44).all()), f"{name}: qx outside its bound"
    assert torch.equal(flags.bool(), ref["flags"]), f"{name}: flags {flags.tolist()} != {ref['flags'].tolist()}"
    assert bool((resid[~rejected] == -1).all()), f"{name}: resid is -1 where the draft was accepted"
    tok = resid.long().clamp_min(0)[..., None]
    assert bool((ref["may"].gather(-1, tok)[..., 0] & (resid >= 0))[rejected].all()), f"{name}: residual token {resid.tolist()}"
    lead = flags.long().cumprod(1).sum(1)
    assert torch.equal(accepted.long(), lead), f"{name}: accepted is the number of leading flags"
    want = torch.where(lead == kk, bonus.long(), resid.long().gather(1, lead.clamp_max(kk - 1)[:, None])[:, 0])
    assert torch.equal(nxt.long(), want), f"{name}: next {nxt.tolist()} != {want.tolist()}"
    assert not bool(flags[-1, -1]) or same, f"{name}: the draft outside the target's survivors was accepted"
    if same:
        assert bool(flags.all()) and torch.equal(nxt, bonus), f"{name}: equal heads accept everything"


def all_cases(dtype, v):
    cases = [(v, dtype, setting, shape, False) for setting in SETTINGS for shape in SHAPES]
    return cases + [SAME] if (v, dtype) == SAME[:2] else cases


def distribution_is_the_targets(verify):
    """v = 11, kk = 1, N = 8192 rows with the same (P, Q), nothing filtered; drafts from q under one key, verified
    under another: the emitted token (the draft if accepted, else resid) has the fp64 p's frequencies within 5
    binomial standard deviations per token.  ``verify(T, D, drafts, t_floor, d_floor, bonus, v, inv_t, key) -> out``."""
    n, v, vp = 8192, 11, 64
    P = torch.tensor([2.0, 0.5, -1.0, 1.5, 0.0, -2.0, 1.0, -0.5, 0.25, -3.0, 0.75])
    Q = P.flip(0).clone()
    p, q = P.double().softmax(-1), Q.double().softmax(-1)
    assert float((p - q).abs().sum() / 2) >= 0.3
    T, D = torch.zeros(n, 2, vp), torch.zeros(n, 1, vp)
    T[..., :v], D[..., :v] = P, Q
    d = fused._lm_sample_torch(D.view(n, vp), v, 1.0, 0, 1.0, KEY_D)
    tt = fused._lm_sample_torch(T.view(-1, vp), v, 1.0, 0, 1.0, KEY_T)
    drafts = d[0].view(n, 1)
    out = verify(T, D, drafts, tt[2].view(n, 2), d[2].view(n, 1), tt[0].view(n, 2)[:, 1].clone(), v, 1.0, KEY)
    flags, resid = out[2].cpu(), out[3].cpu()
    emitted = torch.where(flags.bool(), drafts, resid)[:, 0].long()
    freq = torch.bincount(emitted, minlength=v).double() / n
    assert bool(((freq - p).abs() <= 5 * (p * (1 - p) / n).sqrt()).all()), (freq, p)
