"""Cases, generators, closed forms and checks shared by test_norm_exact_gpu.py
and test_norm_exact_cpu.py (csrc/norm_kernels.hip; docs/TEST_TOLERANCES.md
"Norm, SwiGLU, RoPE and partial sums").

Every ``check_*`` function takes the operation as a callable with the raw
op's signature, so that the GPU tests (the HIP kernels) and the CPU tests (the
fp32 PyTorch emulations ``emul_fwd`` / ``emul_bwd`` below, with and without a
planted defect) run literally the same cases and the same assertions.  The
emulations are the operations' arithmetic written from their definition --
whole-row fp32 sums, no lanes, chunks or folds -- not a port of the kernels."""
import torch

from distributed_lion_pytorch_amd.ops import fused
from numerics import assert_bits, assert_col_partials, assert_rounded, assert_within, drop_consts, tie_share

BF16 = torch.bfloat16
U = 2.0 ** -24  # unit roundoff of fp32

EXACT_WIDTHS = [256, 768, 1024, 2048, 8192]
TAIL_WIDTHS = [264, 520, 1016, 1032, 3584, 7168, 8184]  # 7168: the only way to 7 waves per row, every chunk live
WIDTHS = EXACT_WIDTHS + TAIL_WIDTHS
ROWS = [1, 5, 37]  # not multiples of the 4 rows a block takes at C <= 1024
MEANS = [0, 1, -2, 4, 8]  # row means of the exact-statistics rows: 0 and powers of two (3 fails at 896 / 3584 / 7168)
MIN_TIE_SHARE = 0.10
# (p, with y, with bias); inv_keep is 1, 2 and 4: the scaled branch stays exact
FWD_CONFIGS = [(0.0, False, False), (0.0, True, False), (0.0, True, True), (0.5, True, True), (0.5, True, False),
               (0.75, True, True), (0.75, True, False)]
STATS_CONFIGS = [(0.0, False, False), (0.5, True, True), (0.75, True, False)]
EPS = [1e-5, 0.0]
# (p, want_dy, with dxo_in)
BWD_CONFIGS = [(0.0, False, False), (0.0, True, True), (0.5, True, True), (0.75, True, False)]
BWD_ROWS = 37
BWD_A = [1, -2, 4, 0, 2]   # gd = a + b xh + w: the row's mean of gd and of gd xh
BWD_B = [2, -1, 0, -4, 1]
RSTDS = [0.5, 0.25]


def _seed(*key) -> int:
    s = 29
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return s


def capacity(C: int) -> int:
    """Columns of the instantiation that runs width C: NS * 4 * 64 * WPR >= C."""
    return (C + 255) // 256 * 256 if C <= 1024 else (C + 1023) // 1024 * 1024


def rows_per_block(C: int) -> int:
    """Rows a backward block takes per iteration (RPB): 4 one-wave rows up to C = 1024, else one."""
    return 4 if C <= 1024 else 1


def block_rows(rows: int, C: int, parts: int):
    """Row sets of the backward's partial rows: block b owns rows RPB * (b + parts * j) + grp, grp < RPB."""
    r = torch.arange(rows)
    blk = (r // rows_per_block(C)) % parts
    return [r[blk == b] for b in range(parts)]


def bwd_parts(rows: int, C: int):
    """parts = 1; one that leaves rows for only some row groups of a block's last iteration (RPB = 4) / an
    uneven split (RPB = 1); one larger than the number of row groups (empty blocks)."""
    groups = (rows + rows_per_block(C) - 1) // rows_per_block(C)
    return [1, 3, groups + 2]


def inv_c32(C: int) -> torch.Tensor:
    return torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(C), dtype=torch.float32)


def mean_is_exact(m: int, C: int) -> bool:
    """float32(m * C) * float32(1 / C) == m: the precondition of the exact-statistics rows."""
    return float(torch.tensor(float(m * C), dtype=torch.float32) * inv_c32(C)) == float(m)


def _rn(x32: torch.Tensor, defect=None) -> torch.Tensor:
    """fp32 -> bf16, round to nearest even (``trunc``: the low 16 bits dropped)."""
    if defect == "trunc":
        return (x32.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).to(BF16)
    return x32.to(BF16)


def keep_mask(rows, C, p, seed, device="cpu"):
    th, _ = drop_consts(p)
    if th == 0:
        return torch.ones(rows, C, dtype=torch.bool, device=device)
    return fused.norm_dropout_keep(rows, C, p, seed, device)


def params(C, kind, rms, seed, device="cpu"):
    """gamma / beta: ``pow2`` -- gamma in {1, -1, 2, -2, 0.5}, beta integers in [-4, 4]; ``randn`` -- 1 + 0.1 randn
    and 0.1 randn."""
    g = torch.Generator().manual_seed(_seed(11, C, seed))
    if kind == "pow2":
        gamma = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5])[torch.randint(0, 5, (C,), generator=g)]
        beta = torch.randint(-4, 5, (C,), generator=g).float()
    else:
        gamma = 1 + 0.1 * torch.randn(C, generator=g)
        beta = 0.1 * torch.randn(C, generator=g)
    return gamma.to(BF16).to(device), None if rms else beta.to(BF16).to(device)


# ------------------------------------------------------------------ forward (a): the residual store

def residual_case(C, rows, p, has_y, has_bias, seed=0):
    """Integer x, y, bias (CPU bf16) whose fp32 sum x + inv_keep (y + bias) is an odd integer of magnitude up to
    495 -- a bf16 tie wherever it reaches 256: x = +-(odd in [129, 255]), y = the sign of x times an even number in
    [12, 56], bias even in [-4, 4]."""
    g = torch.Generator().manual_seed(_seed(1, C, rows, int(p * 100), has_y, has_bias, seed))
    sgn = torch.randint(0, 2, (rows, C), generator=g).float() * 2 - 1
    x = sgn * (129 + 2 * torch.randint(0, 64, (rows, C), generator=g).float())
    y = sgn * 2 * torch.randint(6, 29, (rows, C), generator=g).float() if has_y else None
    bias = 2 * torch.randint(-2, 3, (C,), generator=g).float() if has_bias else None
    cv = lambda t: None if t is None else t.to(BF16)  # noqa: E731
    for t in (x, y, bias):
        assert t is None or torch.equal(t.to(BF16).float(), t)
    return cv(x), cv(y), cv(bias)


def residual_expected(x, y, bias, p, seed):
    """(bf16 xo, the fp32 value before its rounding, keep): xo = bf16(x + keep * inv_keep * (y + bias))."""
    rows, C = x.shape
    if y is None:
        return x.clone(), x.float(), torch.ones(rows, C, dtype=torch.bool, device=x.device)
    _, inv = drop_consts(p)
    keep = keep_mask(rows, C, p, seed, x.device)
    s = y.float() + (bias.float() if bias is not None else 0.0)
    v = x.float() + torch.where(keep, s * inv, torch.zeros((), device=x.device))
    assert torch.equal(v.double(), x.double() + torch.where(keep, s.double() * inv, torch.zeros((), dtype=torch.float64,
                                                                                                 device=x.device)))
    return v.to(BF16), v, keep


def check_h(h, xo, mean, rstd, gamma, beta, name):
    """(c): h against fp64 (xo - mean) rstd gamma + beta evaluated with the operation's own xo, mean and rstd (each
    judged on its own elsewhere).  Floor 2^-21 (|(xo - mean) rstd gamma| + |beta|): four fp32 roundings, doubled."""
    t = (xo.double() - mean.double()[:, None]) * rstd.double()[:, None] * gamma.double()
    b = beta.double() if beta is not None else torch.zeros((), dtype=torch.float64, device=h.device)
    return assert_rounded(h, t + b, 2.0 ** -21 * (t.abs() + b.abs()), f"{name} h")


def check_fwd_residual(run, C, rms, rows, cfg, kind, device, seed=4242):
    """(a) + (c) of one case.  ``run`` has add_norm_fwd's signature.  Returns the tie share."""
    p, has_y, has_bias = cfg
    name = f"fwd C={C} rms={rms} rows={rows} p={p} y={has_y} bias={has_bias}"
    x, y, bias = (None if t is None else t.to(device) for t in residual_case(C, rows, p, has_y, has_bias))
    gamma, beta = params(C, kind, rms, 1, device)
    x_in = x.clone()
    exp, v32, keep = residual_expected(x, y, bias, p, seed)
    xo, h, mean, rstd = run(x, y, bias, gamma, beta, 1e-5, rms, p, seed)
    assert xo.shape == x.shape and h.shape == x.shape and mean.shape == (rows,) and rstd.shape == (rows,)
    assert_bits(xo, exp, f"{name} xo")
    assert_bits(x if has_y else xo, x_in, f"{name} x")  # the input is left alone; without y, xo is x
    share = 1.0
    if has_y:
        assert_bits(xo[~keep], x_in[~keep], f"{name} dropped positions")
        share = tie_share(v32.double())
        assert share >= MIN_TIE_SHARE, f"{name}: only {share:.3f} of the sums are bf16 ties"
    s = exp.float().sum(-1)  # integers: exact in any order
    assert float(exp.double().abs().sum(-1).max()) < 2.0 ** 24
    exp_mean = torch.zeros_like(s) if rms else s * inv_c32(C).to(device)
    assert_bits(mean, exp_mean, f"{name} mean")
    check_h(h, xo, mean, rstd, gamma, beta, name)
    return share


# ------------------------------------------------------------------ forward (b): exact statistics

def stats_case(C, rows, p, has_y, has_bias, seed=4242):
    """Target rows xo = m + d with integer |d| <= 16, sum d = 0 (the second half of a row is minus the first half,
    rotated), m = MEANS[row % 5]; x = xo - keep * inv_keep * (y + bias) with |y| <= 40, |bias| <= 8."""
    g = torch.Generator().manual_seed(_seed(2, C, rows, int(p * 100), has_y, has_bias))
    half = torch.randint(-16, 17, (rows, C // 2), generator=g).float()
    d = torch.cat([half, -half.roll(3, 1)], 1)
    m = torch.tensor([float(MEANS[i % len(MEANS)]) for i in range(rows)])
    xo = m[:, None] + d
    y = torch.randint(-40, 41, (rows, C), generator=g).float() if has_y else None
    bias = torch.randint(-8, 9, (C,), generator=g).float() if has_bias else None
    x = xo
    if has_y:
        _, inv = drop_consts(p)
        s = y + (bias if bias is not None else 0.0)
        x = xo - torch.where(keep_mask(rows, C, p, seed), s * inv, torch.zeros(()))
    for t in (x, y, bias, xo):
        assert t is None or torch.equal(t.to(BF16).float(), t), "operand not exact in bf16"
    cv = lambda t: None if t is None else t.to(BF16)  # noqa: E731
    return cv(x), cv(y), cv(bias), cv(xo), m, d


def check_fwd_stats(run, C, rms, rows, cfg, eps, kind, device, seed=4242):
    """(b) + (c): xo is the target bit for bit, mean is m exactly, rstd within 2^-21 of fp64 1 / sqrt(q / C + eps)
    with q = sum (xo - mean)^2 an exact integer below 2^24.  Returns the worst |rstd - ref| / (2^-21 ref)."""
    p, has_y, has_bias = cfg
    name = f"stats C={C} rms={rms} rows={rows} p={p} y={has_y} eps={eps}"
    x, y, bias, xo_t, m, d = stats_case(C, rows, p, has_y, has_bias, seed)
    x, y, bias, xo_t = (None if t is None else t.to(device) for t in (x, y, bias, xo_t))
    gamma, beta = params(C, kind, rms, 2, device)
    assert all(mean_is_exact(int(v), C) for v in m.tolist())
    xo, h, mean, rstd = run(x, y, bias, gamma, beta, eps, rms, p, seed)
    assert_bits(xo, xo_t, f"{name} xo")
    q = (xo_t.double() ** 2).sum(-1) if rms else (d.double() ** 2).sum(-1).to(device)
    assert float(q.max()) < 2.0 ** 24 and float(q.min()) > 0
    assert_bits(mean, torch.zeros_like(mean) if rms else m.to(device), f"{name} mean")
    ref = 1.0 / torch.sqrt(q / C + eps)
    worst = assert_within(rstd, ref, 2.0 ** -21 * ref, f"{name} rstd")
    check_h(h, xo, mean, rstd, gamma, beta, name)
    return worst


# ------------------------------------------------------------------ forward (d): randn rows far from zero

def offset_case(C, rows, has_y, seed=0):
    """randn rows whose mean is 3, 4 or 5 standard deviations from zero, on either side."""
    g = torch.Generator().manual_seed(_seed(3, C, rows, has_y, seed))
    off = torch.tensor([(3.0 + i % 3) * (1 if i % 2 == 0 else -1) for i in range(rows)])
    x = (off[:, None] + torch.randn(rows, C, generator=g)).to(BF16)
    y = (0.5 * torch.randn(rows, C, generator=g)).to(BF16) if has_y else None
    bias = (0.1 * torch.randn(C, generator=g)).to(BF16) if has_y else None
    return x, y, bias


def stats_bounds(xo, eps, rms):
    """fp64 (mean, e_mean, rstd, e_rstd) of the rows of xo; the derivation is in docs/TEST_TOLERANCES.md.
    mean: an fp32 sum of C terms in any order, the rounding of 1 / C and the product: (C + 2) 2^-24 sum |x| / C.
    var: each term (x - mean)^2 carries three roundings and the sum C more, the error of the mean enters as
    e_mean^2 (the cross term vanishes): (C + 5) 2^-24 var + e_mean^2, then one rounding for + eps.
    rstd: relative r / (2 (1 - r)) with r the relative error of var + eps, plus 2^-23 for the root."""
    x = xo.double()
    C = x.shape[1]
    if rms:
        mean, e_mean = torch.zeros_like(x[:, 0]), torch.zeros_like(x[:, 0])
    else:
        mean, e_mean = x.mean(-1), (C + 2) * U * x.abs().sum(-1) / C
    var = ((x - mean[:, None]) ** 2).mean(-1)
    e_var = (C + 5) * U * var + e_mean ** 2 + U * (var + eps)
    r = e_var / (var + eps)
    assert float(r.max()) < 0.5
    rstd = 1.0 / torch.sqrt(var + eps)
    return mean, e_mean, rstd, rstd * (0.5 * r / (1 - r) + 2.0 ** -23)


def check_fwd_offset(run, C, rms, rows, has_y, kind, device, seed=77):
    """(d) + (c); the statistics are those of the bf16 xo the operation returned.  Returns the worst ratios."""
    name = f"offset C={C} rms={rms} rows={rows} y={has_y}"
    x, y, bias = (None if t is None else t.to(device) for t in offset_case(C, rows, has_y))
    gamma, beta = params(C, kind, rms, 3, device)
    xo, h, mean, rstd = run(x, y, bias, gamma, beta, 1e-5, rms, 0.5 if has_y else 0.0, seed)
    if not has_y:
        assert_bits(xo, x, f"{name} xo")
    m64, e_m, r64, e_r = stats_bounds(xo, 1e-5, rms)
    if rms:
        assert_bits(mean, torch.zeros_like(mean), f"{name} mean")
        wm = 0.0
    else:
        wm = assert_within(mean, m64, e_m, f"{name} mean")
    wr = assert_within(rstd, r64, e_r, f"{name} rstd")
    check_h(h, xo, mean, rstd, gamma, beta, name)
    return wm, wr


# ------------------------------------------------------------------ backward: exact rows

def bwd_case(C, rows, rms, with_dxo, seed=0):
    """mean integer (0 for RMS), rstd in {0.5, 0.25}, xo = mean + s / rstd with balanced signs s (xh = s exactly),
    gamma a power of two, dh = (a + b s + w) / gamma with integer w orthogonal to 1 and to s and different in every
    column, dxo_in = rstd * (even integer in +-[272, 494]).  Returns the operands and (t, dh * xh): t = the fp32
    value dx rounds, rstd * (D + w) for LayerNorm and rstd * (D + a + w) for RMS (m1 is forced to 0)."""
    g = torch.Generator().manual_seed(_seed(4, C, rows, rms, with_dxo, seed))
    mean = torch.tensor([0.0 if rms else float(MEANS[i % 5]) for i in range(rows)])
    rstd = torch.tensor([RSTDS[i % 2] for i in range(rows)])
    a = torch.tensor([float(BWD_A[i % 5]) for i in range(rows)])
    b = torch.tensor([float(BWD_B[(i // 2) % 5]) for i in range(rows)])
    sh = torch.randint(0, 2, (rows, C // 2), generator=g).float() * 2 - 1
    s = torch.cat([sh, -sh], 1)                                    # sum s = 0
    r = torch.randint(-6, 7, (rows, C // 4), generator=g).float() + (torch.arange(C // 4) % 7).float() - 3
    t = torch.cat([r, -r.roll(1, 1)], 1)                           # sum t = 0
    w = torch.cat([t, t], 1)                                       # sum w = 0 and sum w s = 0
    assert bool((w.sum(-1) == 0).all()) and bool(((w * s).sum(-1) == 0).all()) and bool((s.sum(-1) == 0).all())
    gamma = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5])[torch.randint(0, 5, (C,), generator=g)]
    gd = a[:, None] + b[:, None] * s + w
    dh = gd / gamma
    xo = mean[:, None] + s / rstd[:, None]
    D = None
    if with_dxo:
        D = (2 * torch.randint(136, 248, (rows, C), generator=g).float()) * (torch.randint(0, 2, (rows, C), generator=g) * 2 - 1)
    inner = w + (a[:, None] if rms else 0.0) + (D if with_dxo else 0.0)
    tval = rstd[:, None] * inner
    dxo = rstd[:, None] * D if with_dxo else None
    for v in (dh, xo, gamma, dxo):
        assert v is None or torch.equal(v.to(BF16).float(), v), "operand not exact in bf16"
    cv = lambda v: None if v is None else v.to(BF16)  # noqa: E731
    return dict(dh=cv(dh), dxo=cv(dxo), xo=cv(xo), gamma=cv(gamma), mean=mean, rstd=rstd, a=a, b=b, s=s, gd=gd, t=tval)


def bwd_means_exact(C):
    """fp32 s1 * inv_c and s2 * inv_c give a and b exactly for every constant used at this width."""
    return all(mean_is_exact(v, C) for v in BWD_A + BWD_B)


def check_bwd_exact(run, C, rms, rows, cfg, parts, device, seed=4242):
    """dx, dy bit-exact with the closed form, the three sections of part per block.  Returns the tie share of dx."""
    p, want_dy, with_dxo = cfg
    name = f"bwd C={C} rms={rms} rows={rows} p={p} dy={want_dy} dxo={with_dxo} parts={parts}"
    c = bwd_case(C, rows, rms, with_dxo)
    assert bwd_means_exact(C)
    dev = lambda v: None if v is None else v.to(device)  # noqa: E731
    dx, dy, part = run(dev(c["dh"]), dev(c["dxo"]), dev(c["xo"]), dev(c["gamma"]), dev(c["mean"]), dev(c["rstd"]), rms, p,
                       seed, want_dy, parts)
    t = c["t"]
    assert_bits(dx.cpu(), t.to(BF16), f"{name} dx")
    share = tie_share(t.double())
    if with_dxo:
        assert share >= MIN_TIE_SHARE, f"{name}: only {share:.3f} of dx are bf16 ties"
    if want_dy:
        _, inv = drop_consts(p)
        keep = keep_mask(rows, C, p, seed)
        exp_dy = torch.where(keep, (t * inv).to(BF16), torch.zeros((), dtype=BF16))
        assert_bits(dy.cpu(), exp_dy, f"{name} dy")
        dy_stored = dy.cpu()
    else:
        assert dy is None or dy.numel() == 0
        dy_stored = torch.zeros(rows, C, dtype=BF16)
    assert tuple(part.shape) == (parts, 3, C) and part.dtype == torch.float32
    sets = block_rows(rows, C, parts)
    pc = part.cpu()
    dh64 = c["dh"].double()
    assert_col_partials(pc[:, 0], dh64 * c["s"].double(), sets, exact=True, name=f"{name} dgamma")
    assert_col_partials(pc[:, 1], dh64, sets, exact=True, name=f"{name} dbeta")
    assert_col_partials(pc[:, 2], dy_stored, sets, exact=True, name=f"{name} dbias")
    return share


# ------------------------------------------------------------------ backward: randn rows

def bwd_randn_case(C, rows, rms, seed=0):
    g = torch.Generator().manual_seed(_seed(5, C, rows, rms, seed))
    off = torch.tensor([(i % 3) * (1.0 if i % 2 == 0 else -1.0) for i in range(rows)])
    xo = (off[:, None] + torch.randn(rows, C, generator=g)).to(BF16)
    dh = torch.randn(rows, C, generator=g).to(BF16)
    dxo = torch.randn(rows, C, generator=g).to(BF16)
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(BF16)
    x64 = xo.double()
    mean = torch.zeros(rows) if rms else x64.mean(-1).float()
    var = (x64 ** 2).mean(-1) if rms else x64.var(-1, unbiased=False)
    rstd = (1.0 / torch.sqrt(var + 1e-5)).float()
    return xo, dh, dxo, gamma, mean, rstd


def bwd_randn_ref(xo, dh, dxo, gamma, mean, rstd, rms):
    """fp64 (t, floor) of t = dxo + rstd (gd - m1 - xh m2) fed the same fp32 mean and rstd.  gd = dh gamma is exact
    in fp32; xh carries two roundings; m1 and m2 are fp32 sums of C terms in any order times a rounded 1 / C:
    e_m1 = (C + 2) 2^-24 sum |gd| / C, e_m2 = (C + 5) 2^-24 sum |gd xh| / C (each term of m2: three roundings).
    floor = rstd (e_m1 + |xh| e_m2) + 8 * 2^-24 (|dxo| + rstd (|gd| + |m1| + |xh m2|)): the two propagated means
    plus the elementwise roundings (2 in xh, 1 each for gd - m1, xh m2, the difference, the scaling and the final
    add: 7, taken as 8)."""
    C = xo.shape[1]
    m, r = mean.double()[:, None], rstd.double()[:, None]
    xh = (xo.double() - m) * r
    gd = dh.double() * gamma.double()
    m1 = torch.zeros_like(r) if rms else gd.mean(-1, keepdim=True)
    m2 = (gd * xh).mean(-1, keepdim=True)
    e1 = torch.zeros_like(r) if rms else (C + 2) * U * gd.abs().sum(-1, keepdim=True) / C
    e2 = (C + 5) * U * (gd * xh).abs().sum(-1, keepdim=True) / C
    t = dxo.double() + r * (gd - m1 - xh * m2)
    floor = r * (e1 + xh.abs() * e2) + 8 * U * (dxo.double().abs() + r * (gd.abs() + m1.abs() + (xh * m2).abs()))
    return t, floor


def check_bwd_randn(run, C, rms, rows, p, device, seed=99):
    name = f"bwd randn C={C} rms={rms} rows={rows} p={p}"
    xo, dh, dxo, gamma, mean, rstd = bwd_randn_case(C, rows, rms)
    dx, dy, part = run(dh.to(device), dxo.to(device), xo.to(device), gamma.to(device), mean.to(device), rstd.to(device),
                       rms, p, seed, True, 3)
    t, floor = bwd_randn_ref(xo, dh, dxo, gamma, mean, rstd, rms)
    w = assert_rounded(dx.cpu(), t, floor, f"{name} dx")
    _, inv = drop_consts(p)
    keep = keep_mask(rows, C, p, seed).double()
    # dy = bf16(keep inv_keep t): one more rounding for the scaling (exact at inv_keep = 1, 2, 4)
    assert_rounded(dy.cpu(), keep * inv * t, keep * inv * floor + U * (keep * inv * t).abs(), f"{name} dy")
    sets = block_rows(rows, C, 3)
    # dbias is the sum of the bf16 dy that was stored: n 2^-24 sum |dy|
    assert_col_partials(part.cpu()[:, 2], dy.cpu(), sets, name=f"{name} dbias")
    assert_col_partials(part.cpu()[:, 1], dh, sets, name=f"{name} dbeta")
    return w


# ------------------------------------------------------------------ fp32 emulations with switchable defects

FWD_DEFECTS = ["inv_cap", "unmasked_var", "trunc"]
BWD_DEFECTS = ["drop_fold_group", "trunc"]


def emul_fwd(x, y, bias, gamma, beta, eps, rms, p, seed, defect=None):
    """add_norm_fwd from its definition in fp32 PyTorch.  Defects: ``inv_cap`` (1 / capacity instead of 1 / C),
    ``unmasked_var`` (the capacity - C padding zeros each add (0 - mean)^2 to the variance sum), ``trunc``."""
    rows, C = x.shape
    if y is not None:
        _, inv = drop_consts(p)
        s = y.float() + (bias.float() if bias is not None else 0.0)
        xo = _rn(x.float() + torch.where(keep_mask(rows, C, p, seed, x.device), s * inv, torch.zeros(())), defect)
    else:
        xo = x
    v = xo.float()
    cap = capacity(C)
    inv_c = inv_c32(cap if defect == "inv_cap" else C)
    mean = torch.zeros(rows) if rms else v.sum(-1) * inv_c
    d = v - mean[:, None]
    q = (d * d).sum(-1)
    if defect == "unmasked_var":
        q = q + (cap - C) * mean * mean
    rstd = 1.0 / torch.sqrt(q * inv_c + torch.tensor(eps, dtype=torch.float32))
    h = d * rstd[:, None] * gamma.float()
    if beta is not None:
        h = h + beta.float()
    return xo, _rn(h, defect), mean, rstd


def emul_bwd(dh, dxo, xo, gamma, mean, rstd, rms, p, seed, want_dy, parts, defect=None):
    """add_norm_bwd from its definition.  ``drop_fold_group``: where a block folds 4 row groups, the rows of
    group 2 are missing from its partial sums."""
    rows, C = xo.shape
    inv_c = inv_c32(C)
    m = torch.zeros(rows) if rms else mean
    xh = (xo.float() - m[:, None]) * rstd[:, None]
    gd = dh.float() * gamma.float()
    m1 = torch.zeros(rows) if rms else gd.sum(-1) * inv_c
    m2 = (gd * xh).sum(-1) * inv_c
    t = rstd[:, None] * (gd - m1[:, None] - xh * m2[:, None])
    if dxo is not None:
        t = dxo.float() + t
    dx = _rn(t, defect)
    dy = None
    stored = torch.zeros(rows, C)
    if want_dy:
        _, inv = drop_consts(p)
        dy = torch.where(keep_mask(rows, C, p, seed), _rn(t * inv, defect), torch.zeros((), dtype=BF16))
        stored = dy.float()
    part = torch.zeros(parts, 3, C)
    rpb = rows_per_block(C)
    for b, idx in enumerate(block_rows(rows, C, parts)):
        if defect == "drop_fold_group" and rpb == 4:
            idx = idx[idx % 4 != 2]
        part[b, 0] = (dh.float() * xh)[idx].sum(0)
        part[b, 1] = dh.float()[idx].sum(0)
        part[b, 2] = stored[idx].sum(0)
    return dx, dy, part



# ------------------------------------------------------------------ the case lists both test files run

CASES = [(C, rms) for C in WIDTHS for rms in (False, True)]
FWD_CASES = [(C, rms, rows) for C, rms in CASES for rows in ROWS]


def _kind(i):
    return "pow2" if i % 2 == 0 else "randn"


def run_fwd_residual(run, C, rms, rows, device):
    return min(check_fwd_residual(run, C, rms, rows, cfg, _kind(i), device) for i, cfg in enumerate(FWD_CONFIGS))


def run_fwd_stats(run, C, rms, device):
    return max(check_fwd_stats(run, C, rms, rows, cfg, eps, _kind(i + j), device)
               for rows in (5, 37) for i, cfg in enumerate(STATS_CONFIGS) for j, eps in enumerate(EPS))


def run_fwd_offset(run, C, rms, device):
    w = [check_fwd_offset(run, C, rms, 6, has_y, _kind(i), device) for i, has_y in enumerate((False, True))]
    return max(a for a, _ in w), max(b for _, b in w)


def run_bwd_exact(run, C, rms, device):
    shares = [check_bwd_exact(run, C, rms, BWD_ROWS, cfg, parts, device)
              for cfg in BWD_CONFIGS for parts in bwd_parts(BWD_ROWS, C)]
    check_bwd_exact(run, C, rms, 1, BWD_CONFIGS[1], 2, device)
    return min(s for s, cfg in zip(shares, [c for c in BWD_CONFIGS for _ in range(3)]) if cfg[2])


def run_bwd_randn(run, C, rms, device):
    return max(check_bwd_randn(run, C, rms, 9, p, device) for p in (0.0, 0.5))
