"""Cases, generators, closed forms and checks shared by test_elementwise_exact_gpu.py
and test_elementwise_exact_cpu.py: SwiGLU, RoPE, the fp32 partial-sum reductions and
the column sums of csrc/elementwise_kernels.hip (docs/TEST_TOLERANCES.md "Norm,
SwiGLU, RoPE and partial sums").

As in norm_exact_cases.py every ``check_*`` takes the operations as callables, so
the GPU tests (the kernels) and the CPU tests (the fp32 PyTorch emulations below,
with and without a planted defect) run the same cases and the same assertions."""
import types

import torch

from numerics import MIN_NORMAL, assert_bits, assert_col_partials, assert_rounded_uflow, strided_rows, tie_share

BF16 = torch.bfloat16
U = 2.0 ** -24
MIN_TIE_SHARE = 0.10


def _seed(*key) -> int:
    s = 31
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return s


def _rn(x32, defect=None):
    if defect == "trunc":
        return (x32.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).to(BF16)
    return x32.to(BF16)


# ------------------------------------------------------------------ SwiGLU

SWIGLU_F = [8, 96, 1376]
SWIGLU_ROWS = [1, 257]
SWIGLU_T = [(64, 64), (64, 192), (128, 64), (128, 192)]  # (rows, F) of the transposing kernels
SENTINEL = 2.0 ** 15
# the zero of silu' lies at g = -1.27846...; its bf16 neighbours are 163 / 128 and 164 / 128
CRAFTED = [0.0, 2.0 ** -10, -2.0 ** -10, -1.2734375, -1.28125, 20.0, -20.0, 60.0, -60.0, -87.0, -89.0, -200.0]
# fp32 roundings of the kernels' expressions (docs): sigmoid = rcp(1 + exp2(-g log2 e)) has 4
N_ROUND_H = 6    # sigmoid, g * s, * u
N_ROUND_DU = 6   # sigmoid, dh * g, * s
N_ROUND_DG = 10  # sigmoid, dh * u, * s, 1 - s, g * (.), 1 + (.), the last product


def swiglu_operands(rows, F, layout="contiguous", device="cpu"):
    """g = 3 randn with every third element (flat index) one of CRAFTED in turn, u and dh randn; bf16.
    ``halves``: g and u are the two halves of a [rows, 2F + 8] buffer whose 8 spare columns hold 2^15."""
    gen = torch.Generator().manual_seed(_seed(1, rows, F))
    g = 3 * torch.randn(rows, F, generator=gen)
    flat = g.view(-1)
    idx = torch.arange(0, flat.numel(), 3)
    flat[idx] = torch.tensor(CRAFTED)[(idx // 3) % len(CRAFTED)]
    u = torch.randn(rows, F, generator=gen)
    dh = torch.randn(rows, F, generator=gen)
    g, u, dh = g.to(BF16).to(device), u.to(BF16).to(device), dh.to(BF16).to(device)
    if layout == "halves":
        buf = torch.full((rows, 2 * F + 8), SENTINEL, dtype=BF16, device=device)
        buf[:, :F], buf[:, F:2 * F] = g, u
        g, u = buf[:, :F], buf[:, F:2 * F]
        return g, u, dh, buf
    return g, u, dh, None


def swiglu_ref(g, u, dh):
    """fp64 (h, dg, du) and their floors k 2^-24 x (the expression with every factor and term replaced by its
    magnitude), k = 2 x the fp32 roundings of the kernel's expression + 2 |g| (the rounding of the exponent's
    argument g log2 e, amplified by the exponential)."""
    g64, u64, d64 = g.double(), u.double(), dh.double()
    s = torch.sigmoid(g64)
    h = g64 * s * u64
    du = d64 * g64 * s
    dg = d64 * u64 * s * (1 + g64 * (1 - s))
    ag = g64.abs()
    f_h = (2 * N_ROUND_H + 2 * ag) * U * h.abs()
    f_du = (2 * N_ROUND_DU + 2 * ag) * U * du.abs()
    f_dg = (2 * N_ROUND_DG + 2 * ag) * U * (d64 * u64).abs() * s * (1 + ag * (1 + s))
    return (h, dg, du), (f_h, f_dg, f_du)


def check_swiglu(ops, rows, F, layout, device):
    """swiglu_fwd, swiglu_bwd and swiglu_bwd_fused against fp64.  Returns the worst err / bound of (h, dg, du)."""
    name = f"swiglu rows={rows} F={F} {layout}"
    g, u, dh, buf = swiglu_operands(rows, F, layout, device)
    keep = None if buf is None else buf.clone()
    (h64, dg64, du64), (f_h, f_dg, f_du) = swiglu_ref(g, u, dh)
    h = ops.swiglu_fwd(g, u)
    dg, du = ops.swiglu_bwd(dh, g, u)
    dgu = ops.swiglu_bwd_fused(dh, g, u)
    assert h.shape == (rows, F) and h.is_contiguous() and dgu.shape == (rows, 2 * F)
    w = (assert_rounded_uflow(h, h64, f_h, f"{name} h"), assert_rounded_uflow(dg, dg64, f_dg, f"{name} dg"),
         assert_rounded_uflow(du, du64, f_du, f"{name} du"))
    assert_bits(dgu[:, :F].contiguous(), dg, f"{name} fused dg")
    assert_bits(dgu[:, F:].contiguous(), du, f"{name} fused du")
    if buf is not None:
        assert_bits(buf, keep, f"{name} operand buffer")
    return w


def check_swiglu_t(ops, rows, F, layout, device):
    """swiglu_fwd_t and swiglu_bwd_fused_t: the row-major outputs and the transposed copies against fp64, and the
    transposed copies bit for bit against the row-major ones."""
    name = f"swiglu_t rows={rows} F={F} {layout}"
    g, u, dh, _ = swiglu_operands(rows, F, layout, device)
    (h64, dg64, du64), (f_h, f_dg, f_du) = swiglu_ref(g, u, dh)
    h, ht = ops.swiglu_fwd_t(g, u)
    dgu, dgut = ops.swiglu_bwd_fused_t(dh, g, u)
    assert ht.shape == (F, rows) and dgu.shape == (rows, 2 * F) and dgut.shape == (2 * F, rows)
    assert_rounded_uflow(h, h64, f_h, f"{name} h")
    assert_rounded_uflow(ht, h64.t(), f_h.t(), f"{name} ht")
    ref = torch.cat([dg64, du64], 1)
    fl = torch.cat([f_dg, f_du], 1)
    assert_rounded_uflow(dgu, ref, fl, f"{name} dgu")
    assert_rounded_uflow(dgut, ref.t(), fl.t(), f"{name} dgut")
    assert_bits(ht, h.t().contiguous(), f"{name} ht vs h")
    assert_bits(dgut, dgu.t().contiguous(), f"{name} dgut vs dgu")


def _sigmoid32(g32):
    """The closed form in fp32 in its usual stable arrangement: e / (1 + e) with e = exp(-|g|), mirrored for g > 0
    (1 / (1 + exp(-g)) overflows to 0 from g = -88.8 on, where g sigmoid(g) is still 2e-37)."""
    e = torch.exp(-g32.abs())
    return torch.where(g32 < 0, e / (1 + e), 1 / (1 + e))


def emul_swiglu(defect=None):
    """The five SwiGLU ops as plain fp32 PyTorch evaluations of the closed forms.  Defects: ``no_one_minus_sg``
    (the gate gradient's factor is 1 + g instead of 1 + g (1 - s)), ``trunc``."""
    def fwd(g, u):
        g32 = g.float()
        return _rn(g32 * _sigmoid32(g32) * u.float(), defect)

    def bwd(dh, g, u):
        g32, s = g.float(), _sigmoid32(g.float())
        f = (1 + g32) if defect == "no_one_minus_sg" else (1 + g32 * (1 - s))
        return _rn(dh.float() * u.float() * s * f, defect), _rn(dh.float() * g32 * s, defect)

    def bwd_fused(dh, g, u):
        return torch.cat(bwd(dh, g, u), 1)

    def fwd_t(g, u):
        h = fwd(g, u)
        return h, h.t().contiguous()

    def bwd_fused_t(dh, g, u):
        d = bwd_fused(dh, g, u)
        return d, d.t().contiguous()

    return types.SimpleNamespace(swiglu_fwd=fwd, swiglu_bwd=bwd, swiglu_bwd_fused=bwd_fused, swiglu_fwd_t=fwd_t,
                                 swiglu_bwd_fused_t=bwd_fused_t)


# ------------------------------------------------------------------ RoPE

ROPE_D = [8, 24, 64, 128]
ROPE_H = [1, 5]
ROPE_B, ROPE_T, ROPE_TABLE_ROWS = 2, 7, 10  # B = 2: row % T matters; tables longer than T


def rope_operands(H, D, device="cpu", small=False, seed=0):
    """x, dy [B, T, H, D]: integers of magnitude 24 .. 32 (``small``: up to 3, every output exact in bf16); cos, sin
    [10, D]: independent multiples of 1/8 of magnitude 5/8 .. 1 (``small``: 0 .. 1), the two halves of a row
    different.  Every product and sum is an exact multiple of 1/8 of magnitude up to 64."""
    gen = torch.Generator().manual_seed(_seed(2, H, D, small, seed))
    sign = lambda shape: torch.randint(0, 2, shape, generator=gen).float() * 2 - 1  # noqa: E731
    shape = (ROPE_B, ROPE_T, H, D)
    if small:
        x, dy = (torch.randint(-3, 4, shape, generator=gen).float() for _ in range(2))
        cos, sin = (torch.randint(-8, 9, (ROPE_TABLE_ROWS, D), generator=gen).float() / 8 for _ in range(2))
    else:
        x, dy = (sign(shape) * torch.randint(24, 33, shape, generator=gen).float() for _ in range(2))
        cos, sin = (sign((ROPE_TABLE_ROWS, D)) * torch.randint(5, 9, (ROPE_TABLE_ROWS, D), generator=gen).float() / 8
                    for _ in range(2))
    assert not torch.equal(cos[:, :D // 2], cos[:, D // 2:]) and not torch.equal(sin[:, :D // 2], sin[:, D // 2:])
    return tuple(t.to(BF16).to(device) for t in (x, dy, cos, sin))


def rope_closed(x, cos, sin, inverse):
    """fp64, unrounded.  Forward: oa = a ca - b sa, ob = b cb + a sb (a, b the halves of a head, ca / cb and sa / sb
    the halves of the token's table rows).  Inverse: the exact transpose, oa = a ca + b sb, ob = b cb - a sa."""
    T, hd = x.shape[1], x.shape[-1] // 2
    x64 = x.double()
    a, b = x64[..., :hd], x64[..., hd:]
    c, s = cos.double()[None, :T, None, :], sin.double()[None, :T, None, :]
    ca, cb, sa, sb = c[..., :hd], c[..., hd:], s[..., :hd], s[..., hd:]
    if not inverse:
        return torch.cat([a * ca - b * sa, b * cb + a * sb], -1)
    return torch.cat([a * ca + b * sb, b * cb - a * sa], -1)


def token_strided(x, left=8, right=8, fill=SENTINEL):
    """x [B, T, H, D] as a view into a [B, T, left + H D + right] buffer whose other columns hold ``fill``."""
    B, T, H, D = x.shape
    wide = torch.full((B, T, left + H * D + right), fill, dtype=x.dtype, device=x.device)
    wide[..., left:left + H * D] = x.reshape(B, T, H * D)
    return wide[..., left:left + H * D].unflatten(-1, (H, D)), wide


def check_rope(ops, H, D, device):
    """rope and rope_ in both directions, contiguous and token-strided, bit-exact with one rounding of the closed
    form; the adjoint identity in exact integers; the unit tables.  Returns the smallest tie share."""
    name = f"rope H={H} D={D}"
    x, dy, cos, sin = rope_operands(H, D, device)
    shares = []
    for inverse, src in ((False, x), (True, dy)):
        exact = rope_closed(src, cos, sin, inverse)
        exp = exact.float().to(BF16)
        assert torch.equal(exact.float().double(), exact)
        shares.append(tie_share(exact))
        assert shares[-1] >= MIN_TIE_SHARE, f"{name}: only {shares[-1]:.3f} of the outputs are bf16 ties"
        y = ops.rope(src, cos, sin, inverse)
        assert y.is_contiguous()
        assert_bits(y, exp, f"{name} inverse={inverse}")
        view, wide = token_strided(src)
        before = wide.clone()
        assert_bits(ops.rope(view, cos, sin, inverse), exp, f"{name} inverse={inverse} strided")
        assert_bits(wide, before, f"{name} inverse={inverse} strided source")
        ops.rope_(view, cos, sin, inverse)
        assert_bits(view.contiguous(), exp, f"{name} inverse={inverse} in place")
        pad = torch.ones_like(wide, dtype=torch.bool)
        pad[..., 8:8 + H * D] = False
        assert_bits(wide[pad], before[pad], f"{name} inverse={inverse} sentinels")
        z = src.clone()
        ops.rope_(z, cos, sin, inverse)
        assert_bits(z, exp, f"{name} inverse={inverse} in place, contiguous")
    # <rope(x), dy> == <x, rope^T(dy)> with outputs that are exact in bf16
    xs, dys, cs, sn = rope_operands(H, D, device, small=True)
    fx, bdy = ops.rope(xs, cs, sn, False), ops.rope(dys, cs, sn, True)
    assert torch.equal(fx.double(), rope_closed(xs, cs, sn, False)) and torch.equal(bdy.double(), rope_closed(dys, cs, sn, True))
    lhs, rhs = float((fx.double() * dys.double()).sum()), float((xs.double() * bdy.double()).sum())
    assert lhs == rhs and lhs * 64 == round(lhs * 64), f"{name}: <rope x, dy> = {lhs} but <x, rope^T dy> = {rhs}"
    # unit tables: cos = 1, sin = 0 is the identity; cos = 0, sin = 1 the signed half swap
    one, zero = torch.ones_like(cos), torch.zeros_like(cos)
    hd = D // 2
    for inverse in (False, True):
        assert_bits(ops.rope(x, one, zero, inverse), x, f"{name} identity inverse={inverse}")
        sw = torch.cat([x[..., hd:], -x[..., :hd]], -1) if inverse else torch.cat([-x[..., hd:], x[..., :hd]], -1)
        assert_bits(ops.rope(x, zero, one, inverse), sw + 0.0, f"{name} half swap inverse={inverse}")
    return min(shares)


def emul_rope(defect=None):
    """rope / rope_ from the definition y = x cos + rotate_half(x) sin (inverse: the transpose) in fp32.
    ``wrong_sin_half``: the inverse takes the sine of the output's own half instead of the partner's."""
    def rope(x, cos, sin, inverse):
        T, hd = x.shape[1], x.shape[-1] // 2
        x32 = x.float()
        c, s = cos.float()[None, :T, None, :], sin.float()[None, :T, None, :]
        if not inverse:
            y = x32 * c + torch.cat([-x32[..., hd:], x32[..., :hd]], -1) * s
        elif defect == "wrong_sin_half":
            y = x32 * c + torch.cat([x32[..., hd:] * s[..., :hd], -x32[..., :hd] * s[..., hd:]], -1)
        else:
            z = x32 * s
            y = x32 * c + torch.cat([z[..., hd:], -z[..., :hd]], -1)
        return _rn(y, defect)

    def rope_(x, cos, sin, inverse):
        x.copy_(rope(x, cos, sin, inverse))

    return types.SimpleNamespace(rope=rope, rope_=rope_)


# ------------------------------------------------------------------ partial sums

# (S, n); the last two are not in the list the tests were asked for: they put the S = 64 / 65 switch between the
# flat and the tall kernel where it is reachable (at n = 16384 both sides are tall: n / 4 < 256 S)
PARTIAL_SHAPES = [(2, 2048), (7, 7168), (7, 256), (64, 16384), (65, 16384), (127, 768), (128, 768), (129, 4),
                  (1000, 3076), (130, 8192), (4096, 64), (64, 65536), (65, 65536)]
# (segment heights, n): each height list on the split route (narrow) and on the multi kernel (256 column blocks)
MULTI_CASES = [([1, 33, 95], 768), ([1, 33, 95], 8192), ([200, 8, 64], 3076), ([200, 8, 64], 8192),
               ([8] * 16, 4), ([8] * 16, 8192), ([1, 33, 30], 768)]
FORMS = ["plain", "acc", "scaled0.5", "scaled4", "scaled4_acc", "multi", "multi_acc"]
FILL = 2.0 ** 22  # the other columns of a strided stack
K_TALL_Q, K_TALL_R = 8, 32


def split_factor(n, total_rows):
    """sum_partials_split_factor restated: the number of row slices of the two-pass reduction (1: one pass)."""
    col_blocks = (n // 4 + K_TALL_Q - 1) // K_TALL_Q
    if col_blocks >= 256 or total_rows < 4 * K_TALL_R:
        return 1
    return max(1, min((512 + col_blocks - 1) // col_blocks, total_rows // (2 * K_TALL_R), 64))


def expected_route(S, n, multi=False):
    """The kernel that reduces a stack of S rows (in all) by n columns: ``split`` (two passes), else ``multi`` for
    a list of stacks, else ``tall`` (S > 64 or n / 4 < 256 S) or ``flat``."""
    if split_factor(n, S) > 1:
        return "split"
    if multi:
        return "multi"
    return "tall" if S > 64 or n // 4 < 256 * S else "flat"


def partial_stack(S, n, seed=0, big=True):
    """fp32 [S, n] of integers in [-3, 3], row 0 replaced by +-(272 .. 496) when ``big``; column sums stay below
    2^24 in any order and a good share of them are bf16 ties (odd, magnitude in [256, 512))."""
    gen = torch.Generator().manual_seed(_seed(3, S, n, seed))
    t = torch.randint(-3, 4, (S, n), generator=gen).float()
    if big:
        t[0] = (torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1) * torch.randint(272, 497, (n,), generator=gen).float()
    assert float(t.abs().sum(0).max()) < 2.0 ** 24
    return t


def old_values(n, seed=0):
    """The accumulation target's old value: bf16 multiples of 8 in [-64, 64] (the parity that makes a sum a tie
    survives the addition, also after the scaling by 4)."""
    gen = torch.Generator().manual_seed(_seed(4, n, seed))
    return (8 * torch.randint(-8, 9, (n,), generator=gen).float()).to(BF16)


def strided_stack(t, device):
    """t [S, n] as the middle third of a [S, 3n] buffer whose other columns hold 2^22."""
    S, n = t.shape
    wide = torch.full((S, 3 * n), FILL, dtype=torch.float32, device=device)
    wide[:, n:2 * n] = t.to(device)
    return wide[:, n:2 * n]


def partial_expected(stacks, form, old):
    """(bf16 expected, the exact fp64 value it rounds): one rounding of scale * sum (+ old)."""
    tot = sum(t.double().sum(0) for t in stacks)
    scale = 0.5 if form.startswith("scaled0.5") else 4.0 if form.startswith("scaled4") else 1.0
    val = tot * scale + (old.double() if form.endswith("acc") else 0.0)
    assert float(val.abs().max()) < 2.0 ** 24 and torch.equal(val.float().double(), val)
    return val.float().to(BF16), val


def run_partial_form(ops, stacks, form, old, device):
    """Calls the op of ``form`` on device stacks; returns the bf16 result [n]."""
    n = stacks[0].shape[1]
    out = old.clone().to(device) if form.endswith("acc") else torch.full((n,), 7.0, dtype=BF16, device=device)
    if form == "plain":
        return ops.sum_partials(stacks[0])
    if form == "acc":
        ops.sum_partials_acc_(stacks[0], out)
    elif form.startswith("scaled"):
        s = torch.tensor([0.5 if form.startswith("scaled0.5") else 4.0], dtype=torch.float32, device=device)
        ops.sum_partials_scaled_(stacks[0], s, out, form.endswith("acc"))
    else:
        ops.sum_partials_multi_(list(stacks), out, form.endswith("acc"))
    return out


def check_partials(ops, S, n, strided, device):
    """Every single-stack form at (S, n), and the one-segment multi form; bit-exact.  Returns (route, tie share)."""
    t = partial_stack(S, n)
    old = old_values(n)
    dev = strided_stack(t, device) if strided else t.to(device)
    share = 1.0
    for form in FORMS:
        exp, val = partial_expected([t], form, old)
        share = min(share, tie_share(val))
        got = run_partial_form(ops, [dev], form, old, device)
        assert_bits(got.cpu(), exp, f"partials S={S} n={n} strided={strided} {form}")
    assert share >= MIN_TIE_SHARE, f"partials S={S} n={n}: only {share:.3f} of the sums are bf16 ties"
    return expected_route(S, n), share


def check_partials_multi(ops, heights, n, strided, device):
    """sum_partials_multi_ over separately allocated stacks of unequal height, plain and accumulating."""
    # one +-(272 .. 496) row in all: the sums stay in the tie range
    ts = [partial_stack(h, n, seed=k + 1, big=k == 0) for k, h in enumerate(heights)]
    old = old_values(n)
    devs = [strided_stack(t, device) if strided else t.to(device) for t in ts]
    share = 1.0
    for form in ("multi", "multi_acc"):
        exp, val = partial_expected(ts, form, old)
        share = min(share, tie_share(val))
        got = run_partial_form(ops, devs, form, old, device)
        assert_bits(got.cpu(), exp, f"multi heights={heights} n={n} strided={strided} {form}")
    assert share >= MIN_TIE_SHARE, f"multi heights={heights} n={n}: only {share:.3f} of the sums are bf16 ties"
    return expected_route(sum(heights), n, multi=True), share


def emul_partials(defect=None):
    """The partial-sum ops from their definition: out = bf16(scale * sum_s part[s] (+ out)) in fp32.
    ``skip_split_group``: where the two-pass route applies, the second group of 32 rows of every stack is left out."""
    def total(stacks):
        S, n = sum(t.shape[0] for t in stacks), stacks[0].shape[1]
        acc = torch.zeros(n)
        for t in stacks:
            rows = torch.arange(t.shape[0])
            if defect == "skip_split_group" and split_factor(n, S) > 1:
                rows = rows[(rows // K_TALL_R) != 1]
            acc = acc + t[rows].sum(0)
        return acc

    def sum_partials(part):
        return _rn(total([part]), defect)

    def acc_(part, out):
        out.copy_(_rn(total([part]) + out.float(), defect))

    def scaled_(part, s, out, accumulate):
        v = total([part]) * s[0]
        out.copy_(_rn(v + out.float() if accumulate else v, defect))

    def multi_(parts, out, accumulate):
        v = total(parts)
        out.copy_(_rn(v + out.float() if accumulate else v, defect))

    return types.SimpleNamespace(sum_partials=sum_partials, sum_partials_acc_=acc_, sum_partials_scaled_=scaled_,
                                 sum_partials_multi_=multi_)


# ------------------------------------------------------------------ column sums

COLSUM_N = [8, 520, 8192, 8200, 16384]
COLSUM_ROWS_PARTS = [(3, 7), (7, 7), (100, 7), (1, 1)]


def check_colsum(colsum_partials, N, rows, parts, device):
    gen = torch.Generator().manual_seed(_seed(5, N, rows, parts))
    x = (torch.randint(-64, 65, (rows, N), generator=gen).float() + (torch.arange(N) % 7).float()).to(BF16)
    part = colsum_partials(x.to(device), parts)
    return assert_col_partials(part.cpu(), x, strided_rows(rows, parts), exact=True, name=f"colsum N={N} rows={rows} parts={parts}")


def emul_colsum(x, parts):
    return torch.stack([x.float()[p::parts].sum(0) for p in range(parts)])
