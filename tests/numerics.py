"""Row-wise and elementwise error bounds against fp64 references.

A max-normalised check (max|got - ref| <= tol * max|ref| over the whole
tensor) says nothing about rows whose magnitude is far below the tensor's
maximum: in causal attention the late token rows, in a softmax the small
probabilities.  The helpers here judge every token row (or element) on its
own scale, with the bound anchored on an fp64 reference and on a rounding
model -- the fp64 computation with only the bf16 roundings that any bf16-MFMA
flash algorithm has to perform -- instead of a guessed tolerance.
docs/TEST_TOLERANCES.md has the measured ratios and the constant ``C_ROWS``.

The second half (``int_operand`` onwards) is the exact-arithmetic GEMM
conformance: integer operands whose fp32 sums are exact, so the expected
output is one deterministic rounding and needs no tolerance at all.
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


# ---------------------------------------------------------------------------
# Exact-arithmetic GEMM conformance (tests/test_gemm_exact_*.py,
# docs/TEST_TOLERANCES.md "GEMM").  With small-integer operands (optionally
# scaled by a power of two) every product and every partial sum of a bf16 GEMM
# is exact in fp32 whatever the accumulation order, so the expected output is
# ONE deterministic rounding of an exactly known number and needs no tolerance.

# fp32 holds every integer of magnitude < 2^24
EXACT_FP32 = 2.0 ** 24
# eval_floor = EVAL_MARGIN x the error of a plain fp32 evaluation (fixed, see the doc)
EVAL_MARGIN = 8.0
# classical bound of a recursive fp32 sum of n terms: n * 2^-24 * sum |x_i|
SUM_EPS = 2.0 ** -24
# rows a wave of the NT kernel folds into one bias-gradient partial row
GEMM_SLAB = 128


def int_operand(shape, lo, hi, seed, device, asym="col", scale=1.0):
    """bf16 [rows, cols] of integers in [lo, hi] times ``scale`` (a power of
    two: the values, their products and sums stay exact), drawn from a seeded
    CPU generator so that CPU and GPU tests see the same data.  ``asym`` adds
    (index % 7) to column 0 ("col") or to row 0 ("row"), so that a transposed
    or misplaced element cannot cancel; None adds nothing."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g).float()
    if asym == "col":
        t[:, 0] += (torch.arange(shape[0]) % 7).float()
    elif asym == "row":
        t[0, :] += (torch.arange(shape[1]) % 7).float()
    else:
        assert asym is None, asym
    assert scale > 0 and float(torch.frexp(torch.tensor(float(scale)))[0]) == 0.5, "scale must be a power of two"
    t = t * scale
    out = t.to(torch.bfloat16)
    assert torch.equal(out.float(), t), "operand not exact in bf16"
    return out.to(device)


def _assert_exact(mag64: torch.Tensor, unit: float, what: str):
    """The exactness condition: sum_k |a_k b_k| (>= |any partial sum, in any
    order|) stays below 2^24 units, ``unit`` being the power of two the
    operands' common scale contributes."""
    worst = float(mag64.max()) / unit if mag64.numel() else 0.0
    assert worst < EXACT_FP32, f"{what}: max sum |a b| = {worst:.0f} units >= 2^24, fp32 accumulation is not exact"


def _unit(*ts) -> float:
    """Product of the operands' power-of-two scales: the smallest non-zero |value| of each."""
    u = 1.0
    for t in ts:
        nz = t[t != 0]
        u *= float(nz.abs().min()) if nz.numel() else 1.0
    return min(u, 1.0)


def exact_nt(a, b):
    """fp64 a [M, K] . b [N, K]^T, asserted exact in fp32 (max |sum| < 2^24)."""
    a64, b64 = a.detach().double(), b.detach().double()
    s = a64 @ b64.t()
    _assert_exact(a64.abs() @ b64.abs().t(), _unit(a64, b64), "exact_nt")
    return s


def exact_tn(P, Q):
    """fp64 P [k, M]^T . Q [k, N] (tensors or lists of row segments), asserted exact in fp32."""
    p64 = (torch.cat(list(P)) if isinstance(P, (list, tuple)) else P).detach().double()
    q64 = (torch.cat(list(Q)) if isinstance(Q, (list, tuple)) else Q).detach().double()
    s = p64.t() @ q64
    _assert_exact(p64.abs().t() @ q64.abs(), _unit(p64, q64), "exact_tn")
    return s


def tie_share(sum64: torch.Tensor) -> float:
    """Fraction of the values that are exact bf16 round-to-nearest ties: 9
    significant bits with the last one set (odd integers in [256, 512), values
    = 2 mod 4 in [512, 1024), ...).  Only on those does round-to-nearest-even
    differ from round-half-up / half-away."""
    m, _ = torch.frexp(sum64.detach().double().abs())  # |x| = m 2^e, m in [0.5, 1)
    s = m * 512.0                                       # in [256, 512): 9 bits before the point
    tie = (s == s.floor()) & (s.floor() % 2 == 1)
    return float(tie.double().mean()) if tie.numel() else 0.0


def bf16_half_ulp(ref64: torch.Tensor) -> torch.Tensor:
    """Half a bf16 ulp at |ref| (fp64): 2^(floor(log2 |ref|) - 8); 0 at ref = 0.
    Between 2^-9 |ref| (top of a binade) and 2^-8 |ref| (bottom)."""
    r = ref64.detach().double().abs()
    _, e = torch.frexp(r)  # r = m 2^e, m in [0.5, 1): floor(log2 r) = e - 1
    return torch.where(r > 0, torch.ldexp(torch.ones_like(r), e - 9), torch.zeros_like(r))


_K0, _K1 = 0.7978845608028654, 0.044715  # sqrt(2 / pi), the tanh form's kappa


def gelu_form(u, exact):
    """gelu(u) in u's own dtype: the erf form (exact) or the tanh approximation."""
    if exact:
        return 0.5 * u * (1.0 + torch.erf(u * 0.7071067811865476))
    return 0.5 * u * (1.0 + torch.tanh(_K0 * (u + _K1 * u * u * u)))


def gelu_grad_form(u, exact):
    """d gelu(u) / du in u's own dtype, the closed form matching gelu_form."""
    if exact:
        return 0.5 * (1.0 + torch.erf(u * 0.7071067811865476)) + u * 0.3989422804014327 * torch.exp(-0.5 * u * u)
    t = torch.tanh(_K0 * (u + _K1 * u * u * u))
    return 0.5 * (1.0 + t) + 0.5 * u * (1.0 - t * t) * _K0 * (1.0 + 3.0 * _K1 * u * u)


def gelu64(u, exact):
    return gelu_form(u.detach().double(), exact)


def gelu_grad64(u, exact):
    return gelu_grad_form(u.detach().double(), exact)


def eval_floor(fn, u32: torch.Tensor) -> float:
    """EVAL_MARGIN x max |fn(u32) - fn(fp64(u32))|: the absolute error of a plain
    fp32 PyTorch evaluation of the closed form ``fn`` on the test's own u.  The
    allowance for evaluating the form in fp32 is anchored on the reference's
    arithmetic, never on the kernel's result."""
    u32 = u32.detach().float()
    if u32.numel() == 0:
        return 0.0
    return EVAL_MARGIN * float((fn(u32).double() - fn(u32.double())).abs().max())


def assert_rounded(got, ref64, floor, name=""):
    """Elementwise |got - ref| <= half a bf16 ulp of ref + floor (a float or a
    tensor): ``got`` is the round-to-nearest bf16 of a value within ``floor`` of
    ref.  The half ulp is taken exactly, 2^(floor(log2 |ref|) - 8): the flat
    2^-9 |ref| is half an ulp only at the top of a binade and rejects bf16(ref)
    itself at the bottom (by up to 2x; test_gemm_exact_cpu shows it), so the
    ratio against 2^-9 |ref| + floor is printed next to the asserted one.
    Prints and returns the largest err / bound."""
    g, r = got.detach().double(), ref64.detach().double()
    assert g.shape == r.shape, f"{name}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
    assert torch.isfinite(g).all(), f"{name}: non-finite values"
    err = (g - r).abs()
    fl = floor.detach().double() if torch.is_tensor(floor) else float(floor)
    bound = bf16_half_ulp(r) + fl
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    flat = torch.where(err == 0, torch.zeros_like(err), err / (HALF_ULP_BF16 * r.abs() + fl))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    worst_flat = float(flat.max()) if flat.numel() else 0.0
    # the share of the floor that the error left over after half an ulp takes up (0: rounding alone explains got)
    over = (err - bf16_half_ulp(r)).clamp_min(0.0)
    used = torch.where(over == 0, torch.zeros_like(over), over / (fl if torch.is_tensor(fl) else torch.full_like(over, fl)))
    used = float(used.max()) if used.numel() else 0.0
    print(f"[rounded] {name}: max err / bound {worst:.3f}, floor used {used:.3f} "
          f"(against the flat 2^-9 |ref| + floor: {worst_flat:.3f})")
    if not worst <= 1.0:
        gf, rf, rr = g.reshape(-1), r.reshape(-1), ratio.reshape(-1)
        nbad = int((~(ratio <= 1)).sum())
        rows = _worst(ratio, lambda i, pos: f"  elem {pos}: got {float(gf[i]):.6e}  ref {float(rf[i]):.6e}  "
                      f"err / bound {float(rr[i]):.2f}")
        raise AssertionError(f"{name}: {nbad} of {ratio.numel()} elements over half a bf16 ulp + floor; worst:\n{rows}")
    return worst


def expect_nt(sum64, bias=None):
    """bf16(fp32(sum) + fp32(bias)): the one rounding of the NT GEMM's plain / bias epilogue."""
    s = sum64.float()
    assert torch.equal(s.double(), sum64), "sum not exact in fp32"
    return (s if bias is None else s + bias.float()).to(torch.bfloat16)


def gemm_slabs(M):
    """Row ranges of the NT kernel's bias-gradient partial rows: slab s = part[2 tm + wr]
    covers rows [128 s, 128 s + 128) of [0, M); 2 * ceil(M / 256) slabs, the trailing ones may be empty."""
    return [slice(min(GEMM_SLAB * s, M), min(GEMM_SLAB * (s + 1), M)) for s in range(2 * ((M + 255) // 256))]


def strided_rows(rows, parts):
    """Row sets of bias_gelu_bwd's partial rows: block p walks rows p, p + parts, ..."""
    return [torch.arange(p, max(rows, p), parts) for p in range(parts)]


def assert_col_partials(part, dz, row_sets, nterms=None, exact=False, name=""):
    """part [len(row_sets), N] fp32 against the fp64 column sums of the kernel's
    own bf16 ``dz`` over each row set (slices or index tensors).  ``exact``:
    bit-equal (integer-valued dz, sums below 2^24).  Otherwise per column
    |part[s] - sum dz| <= n * 2^-24 * sum |dz| with n = ``nterms`` (or the row
    set's size): the classical bound of an fp32 sum of n terms in any order.
    A set with no rows has bound 0: its partial row must be exactly zero.
    Prints and returns the largest err / bound."""
    assert part.dtype == torch.float32, part.dtype
    assert tuple(part.shape) == (len(row_sets), dz.shape[1]), \
        f"{name}: part shape {tuple(part.shape)}, expected {(len(row_sets), dz.shape[1])}"
    assert torch.isfinite(part).all(), f"{name}: non-finite partials"
    p64, d64 = part.detach().double(), dz.detach().double()
    worst, bad = 0.0, []
    for s, rows in enumerate(row_sets):
        blk = d64[rows] if isinstance(rows, slice) else d64[rows.to(d64.device)]
        n = blk.shape[0] if nterms is None else nterms
        col, mag = blk.sum(0), blk.abs().sum(0)
        err = (p64[s] - col).abs()
        if blk.shape[0] == 0:
            assert bool((part[s] == 0).all()), f"{name}: partial row {s} has no valid rows but is not zero"
            continue
        if exact:
            assert float(mag.max()) < EXACT_FP32, f"{name}: slab {s} column sums are not exact in fp32"
            bound = torch.zeros_like(col)
        else:
            bound = n * SUM_EPS * mag
        ok = err <= bound
        # exact: the figure is the largest |error| itself
        ratio = err if exact else torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
        worst = max(worst, float(ratio.max()))
        if not bool(ok.all()):
            j = int(torch.argmax(ratio))
            bad.append(f"  partial row {s}: {int((~ok).sum())} columns off; column {j}: got {float(p64[s, j]):.9e}  "
                       f"sum of dz {float(col[j]):.9e}  bound {float(bound[j]):.3e}")
    print(f"[partials] {name}: " + (f"max |err| {worst:g} (bit-exact sums)" if exact else f"max err / bound {worst:.3f}"))
    assert not bad, f"{name}: bias-gradient partials do not match the column sums of dz:\n" + "\n".join(bad[:5])
    return worst


def assert_bits(got, exp, name=""):
    """Bit-equal tensors of one dtype (NaN, the sign of zero and every rounding included)."""
    assert got.shape == exp.shape and got.dtype == exp.dtype, \
        f"{name}: {tuple(got.shape)} {got.dtype} vs {tuple(exp.shape)} {exp.dtype}"
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    same = got.contiguous().view(view) == exp.contiguous().view(view)
    if not bool(same.all()):
        bad = ~same
        diff = (got.double() - exp.double()).abs()[bad]
        i = tuple(int(j) for j in bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ, max |diff| "
                             f"{float(diff.max()):.6g}; first at {i}: got {float(got[i])!r} expected {float(exp[i])!r}")


# ---------------------------------------------------------------------------
# LoRA adapter kernels (tests/test_lora_exact_*.py, docs/TEST_TOLERANCES.md
# "LoRA and 4-bit").  The dropout constants, the row ranges of the fp32
# partials and the checks of the two-operand partial sums.

def drop_consts(p: float):
    """(thresh16, inv_keep) as the bindings derive them from p: an element is
    kept when its 16-bit draw >= thresh16, inv_keep = fp32(65536 / (65536 - thresh16))
    (exactly 2 at p = 0.5 and 4 at p = 0.75)."""
    th = min(65535, int(p * 65536.0 + 0.5))
    return th, float(torch.tensor(65536.0 / (65536.0 - th), dtype=torch.float32))


def lora_parts(rows: int, N: int):
    """(P, rpp, ranges) of lora_cols' partials by the documented rule: P =
    min(512 // cblocks, ceil(rows / 16)) but at least 1 with cblocks = ceil(N /
    512), rpp = ceil(rows / P), part p sums the rows [p rpp, min((p + 1) rpp,
    rows)) -- an empty range where p rpp >= rows."""
    cblocks = (N + 511) // 512
    P = max(1, min(512 // cblocks, (rows + 15) // 16))
    rpp = (rows + P - 1) // P
    return P, rpp, [(min(p * rpp, rows), min((p + 1) * rpp, rows)) for p in range(P)]


def part_sums64(g, y, ranges, layout):
    """fp64 sums over each contiguous row range of g[t, n] * y[t, j] and of
    their magnitudes: [P, N, R] (layout "nr", the layout of B) or [P, R, N]
    ("rn", the layout of A)."""
    assert layout in ("nr", "rn"), layout
    g64, y64 = g.detach().cpu().double(), y.detach().cpu().double()
    rows, P = g64.shape[0], len(ranges)
    rpp = max(max(r1 - r0 for r0, r1 in ranges), 1)
    assert all(r0 == min(p * rpp, rows) and r1 == min((p + 1) * rpp, rows) for p, (r0, r1) in enumerate(ranges))
    pad = max(P * rpp - rows, 0)
    gp = torch.nn.functional.pad(g64, (0, 0, 0, pad))[:P * rpp].view(P, rpp, -1)
    yp = torch.nn.functional.pad(y64, (0, 0, 0, pad))[:P * rpp].view(P, rpp, -1)
    eq = "ptn,ptj->pnj" if layout == "nr" else "ptn,ptj->pjn"
    return torch.einsum(eq, gp, yp), torch.einsum(eq, gp.abs(), yp.abs())


def assert_part_sums(part, g, y, ranges, layout, yscale=1.0, exact=False, name=""):
    """part (fp32, [P, N, R] or [P, R, N]) against yscale * the fp64 sums of
    g[t, n] * y[t, j] over each part's own row range.  ``exact``: bit-equal
    (operands whose sums stay below 2^24 units, yscale a power of two).
    Otherwise |part - ref| <= n * 2^-24 * yscale * sum |g y| with n the rows of
    the range: n - 1 additions in any order and one rounding for the scaling
    (the product of two bf16 is exact in fp32).  A part without rows has bound
    0 either way and must be +0 throughout.  Prints and returns the worst err / bound."""
    assert part.dtype == torch.float32, part.dtype
    s, mag = part_sums64(g, y, ranges, layout)
    assert tuple(part.shape) == tuple(s.shape), f"{name}: part shape {tuple(part.shape)}, expected {tuple(s.shape)}"
    assert torch.isfinite(part).all(), f"{name}: non-finite partials"
    p_cpu = part.detach().cpu()
    empty = torch.tensor([r1 <= r0 for r0, r1 in ranges])
    if bool(empty.any()):
        z = p_cpu[empty]
        assert_bits(z, torch.zeros_like(z), f"{name}: parts without rows")
    if exact:
        _assert_exact(mag, _unit(g.detach().cpu().double(), y.detach().cpu().double()), f"{name}: part sums")
        exp = (s * yscale).float() + 0.0  # a zero sum is +0 in the kernel (the accumulators start at +0)
        assert torch.equal(exp.double(), s * yscale), f"{name}: scaled sums not exact in fp32"
        assert_bits(p_cpu, exp.cpu(), name)
        print(f"[parts] {name}: {len(ranges)} parts ({int(empty.sum())} empty) bit-exact")
        return 0.0
    n = torch.tensor([max(r1 - r0, 0) for r0, r1 in ranges], dtype=torch.float64).view(-1, 1, 1)
    bound = n * SUM_EPS * abs(yscale) * mag.cpu()
    err = (p_cpu.double() - (s * yscale).cpu()).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[parts] {name}: max err / bound {worst:.3f} ({len(ranges)} parts, {int(empty.sum())} empty)")
    if not worst <= 1.0:
        i = tuple(int(j) for j in (ratio > 1).nonzero()[0])
        raise AssertionError(f"{name}: {int((ratio > 1).sum())} of {ratio.numel()} partial sums over n * 2^-24 * sum |terms|; "
                             f"first at {i}: got {float(p_cpu[i]):.9e}  ref {float((s * yscale)[i]):.9e}  "
                             f"bound {float(bound[i]):.3e}")
    return worst


def assert_within(got, ref64, bound, name=""):
    """Elementwise |got - ref| <= bound (an fp64 tensor); prints and returns the worst err / bound."""
    g, r, b = got.detach().double().cpu(), ref64.detach().double().cpu(), bound.detach().double().cpu()
    assert g.shape == r.shape, f"{name}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
    assert torch.isfinite(g).all(), f"{name}: non-finite values"
    err = (g - r).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[within] {name}: max err / bound {worst:.3f}")
    if not worst <= 1.0:
        i = tuple(int(j) for j in (ratio > 1).nonzero()[0])
        raise AssertionError(f"{name}: {int((ratio > 1).sum())} of {ratio.numel()} elements over the bound; first at {i}: "
                             f"got {float(g[i]):.6e}  ref {float(r[i]):.6e}  bound {float(b[i]):.3e}")
    return worst


# ---------------------------------------------------------------------------
# Norm, SwiGLU, RoPE and partial sums (tests/test_norm_exact_*.py,
# tests/test_elementwise_exact_*.py, docs/TEST_TOLERANCES.md).

# the smallest normal fp32 (and bf16) number: below it the kernels' exp2 / rcp flush to zero
MIN_NORMAL = 2.0 ** -126


def assert_rounded_uflow(got, ref64, floor, name=""):
    """assert_rounded, except that an element whose reference is below 2^-126 (the smallest normal fp32 and bf16
    number) may be zero or the reference: it is judged against 0 when it is 0, and otherwise with half the spacing
    of the bf16 subnormals (2^-134) added to its bound."""
    tiny = ref64.abs() < MIN_NORMAL
    zero = tiny & (got.double() == 0)
    ref = torch.where(zero, torch.zeros_like(ref64), ref64)
    fl = floor + torch.where(tiny & ~zero, torch.full_like(ref64, 2.0 ** -134), torch.zeros_like(ref64))
    return assert_rounded(got, ref, fl, name)
