"""Row-wise and elementwise error bounds against fp64 references.

A max-normalised check (max|got - ref| <= tol * max|ref| over the whole
tensor) says nothing about rows whose magnitude is far below the tensor's
maximum: in causal attention the late token rows, in a softmax the small
probabilities.  The helpers here judge every token row (or element) on its
own scale, with the bound anchored on an fp64 reference and on a rounding
model -- the fp64 computation with only the bf16 roundings that any bf16-MFMA
flash algorithm has to perform -- instead of a guessed tolerance.
docs/TEST_TOLERANCES.md has the measured ratios and the constant ``C_ROWS``.
"""
import torch

from distributed_lion_pytorch_amd.ops import fused

# half a bf16 ulp of a row's largest element, relative to it
HALF_ULP_BF16 = 2.0 ** -9
# rows that are zero by construction are judged on this fraction of dV's row max
ZERO_FLOOR = 2.0 ** -7
# got's row error may be C_ROWS x the rounding model's.  Not taken from the
# kernels' results: docs/TEST_TOLERANCES.md has the derivation (a second exact
# realisation of the model's own rounding set reaches 4.3) and the measured table
C_ROWS = 8.0


def _rows(t: torch.Tensor) -> torch.Tensor:
    """[B, T, ...] -> fp64 [B, T, rest]; a 2-D tensor's rows are its dim 0."""
    t = t.detach().double()
    return t.reshape(t.shape[0], t.shape[1], -1) if t.dim() >= 3 else t.reshape(t.shape[0], -1)


def row_err(got: torch.Tensor, ref64: torch.Tensor) -> torch.Tensor:
    """Per token row max_d |got - ref| ([B, T] for [B, T, H, D] / [B, T, H*D])."""
    return (_rows(got) - _rows(ref64)).abs().amax(-1)


def row_max(ref64: torch.Tensor) -> torch.Tensor:
    """Per token row max_d |ref|."""
    return _rows(ref64).abs().amax(-1)


def rows_ratio(got, ref64, model, zero_floor=None) -> torch.Tensor:
    """Per row: (row_err(got) - zero_floor)+ / max(row_err(model), 2^-9 row_max(ref))."""
    err = row_err(got, ref64)
    if zero_floor is not None:
        err = (err - zero_floor).clamp_min(0.0)
    base = torch.maximum(row_err(model, ref64), HALF_ULP_BF16 * row_max(ref64))
    ratio = err / base
    return torch.where(err == 0, torch.zeros_like(ratio), ratio)  # 0 / 0: an exact row


def _worst(score: torch.Tensor, lines, n=5) -> str:
    flat = score.reshape(-1)
    idx = torch.argsort(flat, descending=True)[:n].tolist()
    return "\n".join(lines(i, tuple(int(j) for j in torch.unravel_index(torch.tensor(i), score.shape))) for i in idx)


def assert_rows_close(got, ref64, model, c, zero_floor=None, name=""):
    """Every row i: row_err(got)[i] <= c * max(row_err(model)[i], 2^-9 row_max(ref)[i]) + zero_floor[i].

    ``model`` is the rounding model's result (attention_ref64(..., model=True)),
    ``zero_floor`` ([B, T] or None) is non-zero only on rows whose reference is
    zero by construction.  Prints and returns the largest ratio
    row_err(got) / max(row_err(model), 2^-9 row_max), the figure c bounds."""
    assert torch.isfinite(_rows(got)).all(), f"{name}: non-finite values"
    ratio = rows_ratio(got, ref64, model, zero_floor)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[rows] {name}: max ratio {worst:.3f} (c = {c:g})")
    if worst > c:
        err, merr, rmax = row_err(got, ref64).reshape(-1), row_err(model, ref64).reshape(-1), row_max(ref64).reshape(-1)
        nbad = int((ratio > c).sum())
        rows = _worst(ratio, lambda i, pos: f"  row {pos}: err {float(err[i]):.3e}  model err {float(merr[i]):.3e}  "
                      f"row max {float(rmax[i]):.3e}  ratio {float(ratio.reshape(-1)[i]):.2f}")
        raise AssertionError(f"{name}: {nbad} of {ratio.numel()} rows over c = {c:g} x the rounding model; "
                             f"worst:\n{rows}")
    return worst


def assert_elems_close(got, ref64, rtol, atol, name=""):
    """Elementwise |got - ref| <= rtol |ref| + atol; prints and returns the largest err / bound."""
    g, r = got.detach().double(), ref64.detach().double()
    assert torch.isfinite(g).all(), f"{name}: non-finite values"
    err = (g - r).abs()
    bound = rtol * r.abs() + atol
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[elems] {name}: max err / bound {worst:.3f}")
    if worst > 1.0:
        gf, rf, rr = g.reshape(-1), r.reshape(-1), ratio.reshape(-1)
        nbad = int((ratio > 1).sum())
        rows = _worst(ratio, lambda i, pos: f"  elem {pos}: got {float(gf[i]):.6e}  ref {float(rf[i]):.6e}  "
                      f"err / bound {float(rr[i]):.2f}")
        raise AssertionError(f"{name}: {nbad} of {ratio.numel()} elements over rtol {rtol:g}; worst:\n{rows}")
    return worst


def vec_atol(ref64: torch.Tensor, tol: float) -> float:
    """atol of a 1-D tensor (a column sum): tol x the MEAN magnitude -- an element
    that cancels to near zero keeps the absolute rounding error of its summands."""
    return tol * float(ref64.detach().double().abs().mean())


def _bf16(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).double()


def _rope64(x, cos, sin):
    """fused.rope_reference in fp64: x [B, T, H, D], tables [>= T, D]."""
    T, d2 = x.shape[1], x.shape[-1] // 2
    c, s = cos.double()[None, :T, None, :], sin.double()[None, :T, None, :]
    return x * c + torch.cat([-x[..., d2:], x[..., :d2]], -1) * s


def _rope64_bwd(dy, cos, sin):
    """The transpose of _rope64 (its gradient with respect to x)."""
    T, d2 = dy.shape[1], dy.shape[-1] // 2
    c, s = cos.double()[None, :T, None, :], sin.double()[None, :T, None, :]
    z = dy * s
    return dy * c + torch.cat([z[..., d2:], -z[..., :d2]], -1)


def attention_ref64(q, k, v, dout, p, seed, window, cos=None, sin=None, model=False):
    """Causal (GQA, sliding-window, dropout) attention forward and backward in
    fp64 on the inputs' device: q [B,T,H,D], k / v [B,T,Hkv,D], dout [B,T,H*D]
    -> (out [B,T,H*D], dq, dk, dv in the inputs' shapes).  The dropout mask is
    the kernels' (fused.attention_dropout_keep); with cos / sin [>= T, D] the
    attention runs on rope(q), rope(k) and dq / dk are rotated back.

    The backward is written out (P, dP, delta = rowsum(dO * O), dS = P (dP -
    delta)) so that ``model=True`` can insert the roundings every bf16-MFMA
    flash algorithm performs on its matrix operands and results, and nothing
    else: rope(q), rope(k) -> bf16 (MFMA operands); P after the dropout scaling
    -> bf16 before P V and P^T dO; O -> bf16 before delta; dS -> bf16 before
    dS K and dS^T Q; the four results -> bf16.  The softmax, the accumulations
    and the sum over a GQA group's query heads stay in fp64.  It is the
    calibration of the row bound -- neither the kernels nor
    fused.reference_attention."""
    B, T, H, D = q.shape
    Hkv = k.shape[2]
    rep = H // Hkv
    rnd = _bf16 if model else (lambda t: t)
    q64, k64, v64 = q.detach().double(), k.detach().double(), v.detach().double()
    if cos is not None:
        q64, k64 = rnd(_rope64(q64, cos, sin)), rnd(_rope64(k64, cos, sin))
    qh = q64.transpose(1, 2)  # [B, H, T, D]
    kh = k64.transpose(1, 2).repeat_interleave(rep, dim=1)
    vh = v64.transpose(1, 2).repeat_interleave(rep, dim=1)
    do = dout.detach().double().reshape(B, T, H, D).transpose(1, 2)
    scale = 1.0 / D ** 0.5

    i = torch.arange(T, device=q.device)
    d = i[:, None] - i[None, :]
    visible = (d >= 0) & (d < window) if window else d >= 0
    s = (qh @ kh.transpose(-1, -2)) * scale
    P = torch.softmax(s.masked_fill(~visible, float("-inf")), dim=-1)
    if p > 0:
        th = min(65535, int(round(p * 65536)))
        drop = fused.attention_dropout_keep(B, H, T, p, seed, q.device).double() * (65536.0 / (65536.0 - th))
    else:
        drop = None
    Pd = rnd(P * drop if drop is not None else P)
    O = Pd @ vh

    dv = Pd.transpose(-1, -2) @ do
    dP = do @ vh.transpose(-1, -2)
    if drop is not None:
        dP = dP * drop
    delta = (do * rnd(O)).sum(-1, keepdim=True)
    dS = rnd(P * (dP - delta))
    dq = (dS @ kh) * scale
    dk = (dS.transpose(-1, -2) @ qh) * scale
    # the sum over the query heads of a GQA group stays in fp64
    dk = dk.view(B, Hkv, rep, T, D).sum(2)
    dv = dv.view(B, Hkv, rep, T, D).sum(2)
    out, dq, dk, dv = (t.transpose(1, 2) for t in (O, dq, dk, dv))
    if cos is not None:
        dq, dk = _rope64_bwd(dq, cos, sin), _rope64_bwd(dk, cos, sin)
    return rnd(out).reshape(B, T, H * D), rnd(dq).contiguous(), rnd(dk).contiguous(), rnd(dv).contiguous()


def attention_floors(ref_dq, ref_dv, T, window=0):
    """zero_floor tensors ([B, T]) for dq and dk: dq of query 0 is zero by
    construction (one visible key), and with T == 1 or window == 1 all of dq and
    dk are; those rows are judged on 2^-7 of the same token's dV row max, the
    scale the max-normalised tests use as their floor.  Returns (floor_q, floor_k)."""
    scale = ZERO_FLOOR * row_max(ref_dv)
    if T == 1 or window == 1:
        return scale, scale
    fq = torch.zeros_like(scale)
    fq[:, 0] = scale[:, 0]
    return fq, None


def check_attention(name, got, q, k, v, dout, p, seed, window=0, cos=None, sin=None, c=C_ROWS):
    """assert_rows_close for (out, dq, dk, dv) = got against attention_ref64 and
    its rounding model.  All four ratios are printed before any failure is raised."""
    B, T = q.shape[:2]
    ref = attention_ref64(q, k, v, dout, p, seed, window, cos, sin)
    mod = attention_ref64(q, k, v, dout, p, seed, window, cos, sin, model=True)
    fq, fk = attention_floors(ref[1], ref[3], T, window)
    failures = []
    for g, r, m, f, n in zip(got, ref, mod, (None, fq, fk, None), ("out", "dq", "dk", "dv")):
        try:
            assert_rows_close(g.reshape(B, T, -1), r, m, c, f, f"{name} {n}")
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
