"""The wide-rank LoRA kernels (csrc/lora_wide.hip, r in {32, 64, 128}) one by
one against the closed forms of lora_exact_cases, bit for bit, as
test_lora_exact_gpu.py does for r in {8, 16}: small-integer operands whose fp32
sums are exact (asserted), p in {0, 0.5, 0.75} so that inv_keep is 1, 2 or 4.
Each kernel is judged on its own inputs (lora_up gets the u that lora_rows
returned, lora_cols mode 1 the du that lora_rows returned).  The row ranges of
lora_cols' partials follow the wide rule (fused.lora_cols_parts); the shapes
are explained in lora_wide_cases.  Row-wise cases: randn operands against fp64
references with the bounds of docs/TEST_TOLERANCES.md ("LoRA and 4-bit"),
which are functions of r, K and N."""
import pytest
import torch

from distributed_lion_pytorch_amd.ops import fused, hip
from lora_exact_cases import (BF16, DROPS, MIN_TIE_SHARE, RANDN_P, RANDN_S, RANDN_SHAPES, ROWS_K, ROWS_M, ROWS_M_SWEEP,
                              UP_M, UP_M_SWEEP, UP_N, case_scale, dx_operands, keep_mask, probe_decode, probe_weights,
                              probe_windows, rows_operands, rows_ref, strided, up_operands, up_ref)
from lora_wide_cases import EMPTY_PARTS, ROWS_K_SWEEP, UP_N_SWEEP, WIDE_RANKS, cols_ref_wide, wide_parts
from numerics import (SUM_EPS, assert_bits, assert_part_sums, assert_rounded, assert_within, bf16_half_ulp, drop_consts,
                      tie_share)

pytestmark = pytest.mark.gpu

SEED = 20231


def _ops():
    hip.require()
    return hip.ops()


def _check_rows(cuda, x, a, scale, p, seed, name, view=None):
    """lora_rows on x (or on ``view``, a strided GPU view holding x) against rows_ref; returns the kernel's u."""
    xg = x.to(cuda) if view is None else view
    u = _ops().lora_rows(xg, a.to(cuda), scale, p, seed)
    assert u.shape == (x.shape[0], a.shape[0]) and u.dtype == BF16 and u.is_contiguous()
    assert_bits(u.cpu(), rows_ref(x, a, scale, p, seed), name)
    return u


# ------------------------------------------------------------------ lora_rows
@pytest.mark.parametrize("p", DROPS)
@pytest.mark.parametrize("K", ROWS_K_SWEEP)
@pytest.mark.parametrize("r", WIDE_RANKS)
def test_rows_k_sweep(cuda, r, K, p):
    x, a = rows_operands(ROWS_M, K, r)
    _check_rows(cuda, x, a, case_scale(K, r), p, SEED + K, f"rows M={ROWS_M} K={K} r={r} p={p}")


@pytest.mark.parametrize("p", DROPS)
@pytest.mark.parametrize("M", ROWS_M_SWEEP)
@pytest.mark.parametrize("r", WIDE_RANKS)
def test_rows_m_sweep(cuda, r, M, p):
    x, a = rows_operands(M, ROWS_K, r)
    _check_rows(cuda, x, a, case_scale(M, r), p, SEED + M, f"rows M={M} K={ROWS_K} r={r} p={p}")


@pytest.mark.parametrize("p", DROPS)
@pytest.mark.parametrize("K", [ROWS_K, 4128])
@pytest.mark.parametrize("r", WIDE_RANKS)
def test_rows_strided_x(cuda, r, K, p):
    """x is a column slice (ldin > K) between sentinel columns; the mask index stays t * K + c."""
    x, a = rows_operands(ROWS_M, K, r)
    view = strided(x.to(cuda))
    assert view.stride(0) == K + 24
    _check_rows(cuda, x, a, case_scale(K, r, 1), p, SEED, f"rows strided K={K} r={r} p={p}", view=view)


@pytest.mark.parametrize("N", [32, 768])
@pytest.mark.parametrize("r", WIDE_RANKS)
def test_rows_backward_call(cuda, r, N):
    """du = lora_rows(dout, b^T, s, 0, 0) as _LoraAdd.backward calls it, dout contiguous and strided."""
    _, b, dout = up_operands(UP_M, N, r)
    s = case_scale(N, r)
    bt = b.t().contiguous()
    _check_rows(cuda, dout, bt, s, 0.0, 0, f"rows bwd N={N} r={r}")
    _check_rows(cuda, dout, bt, s, 0.0, 0, f"rows bwd strided N={N} r={r}", view=strided(dout.to(cuda)))


def _probe(cuda, M, K, r, p, seed, scale=2.0, view=False):
    """The forward kernel's keep mask [M, K], every element read back through lora_rows (x = 1)."""
    ones = torch.ones(M, K, dtype=BF16, device=cuda)
    xg = strided(ones) if view else ones
    us = [_ops().lora_rows(xg, probe_weights(K, r, w, cuda), scale, p, seed) for w in range(probe_windows(K, r))]
    return probe_decode(us, K, r, scale, p)


@pytest.mark.parametrize("p", [0.5, 0.75])
@pytest.mark.parametrize("M,K", [(33, 256), (17, 288), (5, 4128)])
@pytest.mark.parametrize("r", WIDE_RANKS)
def test_rows_mask_is_the_host_mask_bit_for_bit(cuda, r, M, K, p):
    host = fused.norm_dropout_keep(M, K, p, SEED)
    got = _probe(cuda, M, K, r, p, SEED)
    assert torch.equal(got, host), f"{int((got != host).sum())} keep bits differ from norm_dropout_keep"
    share = float(host.double().mean())
    assert abs(share - (1 - p)) < 0.05, share


# ------------------------------------------------------- lora_up and lora_cols
def _check_up_cols(cuda, M, N, r, p=0.5, use_strided=False, up=True):
    ops = _ops()
    s = case_scale(M, N, r)
    wrap = (lambda t: strided(t)) if use_strided else (lambda t: t)
    tag = f"M={M} N={N} r={r}" + (" strided" if use_strided else "")
    x, a = rows_operands(M, ROWS_K, r)
    u = _check_rows(cuda, x, a, 1.0, p, SEED, f"u {tag}")  # the kernel's own u feeds up and cols mode 0
    o, b, dout = up_operands(M, N, r)

    if up:
        out = ops.lora_up(wrap(o.to(cuda)), u, b.to(cuda), s)
        exp, inner, total = up_ref(o, u, b, s)
        ti, ts = tie_share(inner), tie_share(total)
        print(f"[ties] up {tag}: adapter term {ti:.3f}, sum {ts:.3f}")
        assert ti >= MIN_TIE_SHARE and ts >= MIN_TIE_SHARE, (ti, ts)
        assert out.is_contiguous()
        assert_bits(out.cpu(), exp, f"up {tag}")

    P, rpp, ranges = wide_parts(M, N, r)
    part, none = ops.lora_cols(wrap(dout.to(cuda)), u, None, s, 0.0, 0)
    assert part.shape == (P, N, r) and part.dtype == torch.float32 and none is None
    assert P * N * r * 4 <= max(M * N * 2, N * r * 4)  # the partials never exceed the g operand (one part aside)
    assert_part_sums(part, dout, u, ranges, "nr", s, exact=True, name=f"cols0 {tag}")
    assert_bits(part.cpu(), cols_ref_wide(dout, u, None, s)[0], f"cols0 ref {tag}")

    # mode 1 at width N: du is the kernel's own, from the backward rows call
    xx, aa, dd, bb = dx_operands(M, N, r)
    du = _check_rows(cuda, dd, bb.t().contiguous(), s, 0.0, 0, f"du {tag}")
    assert bool((du > 0).all())
    for pp in (p, 0.75, 0.0):
        part1, dx = ops.lora_cols(wrap(xx.to(cuda)), du, aa.to(cuda), 1.0, pp, SEED + 1)
        assert part1.shape == (P, r, N) and dx.shape == (M, N) and dx.dtype == BF16
        exp_part, exp_dx = cols_ref_wide(xx, du, aa, 1.0, pp, SEED + 1)
        assert_bits(dx.cpu(), exp_dx, f"dx {tag} p={pp}")
        # strictly positive du and a: dx is non-zero exactly where the mask keeps
        assert torch.equal(dx.cpu() != 0, keep_mask(M, N, pp, SEED + 1)), f"dx mask {tag} p={pp}"
        assert_bits(part1.cpu(), exp_part, f"cols1 {tag} p={pp}")
    return ranges


@pytest.mark.parametrize("N", UP_N_SWEEP)
@pytest.mark.parametrize("r", WIDE_RANKS)
def test_up_cols_n_sweep(cuda, r, N):
    _check_up_cols(cuda, UP_M, N, r)


@pytest.mark.parametrize("M", UP_M_SWEEP)
@pytest.mark.parametrize("r", WIDE_RANKS)
def test_up_cols_m_sweep(cuda, r, M):
    _check_up_cols(cuda, M, UP_N, r)


@pytest.mark.parametrize("r", WIDE_RANKS)
def test_cols_empty_parts(cuda, r):
    """rows = 12801, N = 32.  At r = 32: P = 200 and rpp = 65, so parts 197 .. 199 start past the last row and must
    be +0; at r = 64 / 128 (P = 100 / 50) every part has rows."""
    M, N = EMPTY_PARTS
    ranges = _check_up_cols(cuda, M, N, r, up=False)
    empty = [p for p, (r0, r1) in enumerate(ranges) if r1 <= r0]
    assert len(ranges) == M // (2 * r) and empty == ([197, 198, 199] if r == 32 else [])


@pytest.mark.parametrize("N", [UP_N, 768])
@pytest.mark.parametrize("r", WIDE_RANKS)
def test_up_cols_strided_operands(cuda, r, N):
    """o, dout and x as column slices between sentinel columns (ldo, ldg > N)."""
    _check_up_cols(cuda, UP_M, N, r, use_strided=True)


@pytest.mark.parametrize("r", WIDE_RANKS)
def test_backward_mask_is_the_forward_mask(cuda, r):
    """Same seed, same [M, K]: the elements lora_cols mode 1 zeroes in dx are the ones lora_rows dropped."""
    M, K, p = 37, 288, 0.5
    xx, aa, dd, bb = dx_operands(M, K, r)
    du = _ops().lora_rows(dd.to(cuda), bb.t().contiguous().to(cuda), 2.0, 0.0, 0)
    for view in (False, True):
        fwd = _probe(cuda, M, K, r, p, SEED, view=view)
        xg = strided(xx.to(cuda)) if view else xx.to(cuda)
        _, dx = _ops().lora_cols(xg, du, aa.to(cuda), 1.0, p, SEED)
        assert torch.equal(dx.cpu() != 0, fwd), f"strided={view}"


# ------------------------------------------------- row-wise, realistic operands
@pytest.mark.parametrize("M,K,N", RANDN_SHAPES)
@pytest.mark.parametrize("r", WIDE_RANKS)
def test_lora_kernels_rowwise_fp64(cuda, r, M, K, N):
    ops = _ops()
    p, s, seed = RANDN_P, RANDN_S, 4321
    g = torch.Generator().manual_seed(M + K + N + r)
    x = torch.randn(M, K, generator=g).to(BF16)
    o = torch.randn(M, N, generator=g).to(BF16)
    dout = torch.randn(M, N, generator=g).to(BF16)
    a = (torch.randn(r, K, generator=g) * 0.05).to(BF16)
    b = (torch.randn(N, r, generator=g) * 0.05).to(BF16)
    _, inv = drop_consts(p)
    keep = keep_mask(M, K, p, seed)
    zero = torch.zeros((), dtype=torch.float64)
    tag = f"M={M} K={K} N={N} r={r}"
    xg, ag, bg, dg = x.to(cuda), a.to(cuda), b.to(cuda), dout.to(cuda)

    # forward: xd = bf16(fp32(x) * inv_keep) where kept
    xd = torch.where(keep, (x.float() * inv).to(BF16).double(), zero)
    u = ops.lora_rows(xg, ag, 1.0, p, seed)
    assert_rounded(u.cpu(), xd @ a.double().t(), K * SUM_EPS * (xd.abs() @ a.double().abs().t()), f"u {tag}")

    # out from the kernel's own u: two roundings
    u64 = u.cpu().double()
    out = ops.lora_up(o.to(cuda), u, bg, s)
    inner = s * (u64 @ b.double().t())
    floor = r * SUM_EPS * s * (u64.abs() @ b.double().abs().t())
    total = o.double() + inner
    assert_within(out, total, bf16_half_ulp(inner) + bf16_half_ulp(total) + floor, f"out {tag}")

    # dB partials from the kernel's own u
    P, _, ranges = wide_parts(M, N, r)
    part_b, _ = ops.lora_cols(dg, u, None, s, 0.0, 0)
    assert part_b.shape[0] == P
    assert_part_sums(part_b, dout, u.cpu(), ranges, "nr", s, name=f"dB partials {tag}")

    # du, then dA partials (unrounded x * inv_keep) and dx from the kernel's own du
    du = ops.lora_rows(dg, bg.t().contiguous(), s, 0.0, 0)
    assert_rounded(du.cpu(), s * (dout.double() @ b.double()), N * SUM_EPS * s * (dout.double().abs() @ b.double().abs()),
                   f"du {tag}")
    du64 = du.cpu().double()
    part_a, dx = ops.lora_cols(xg, du, ag, 1.0, p, seed)
    Pa, _, ranges_a = wide_parts(M, K, r)
    assert part_a.shape[0] == Pa
    xs = torch.where(keep, x.double() * inv, zero)
    assert_part_sums(part_a, xs, du64, ranges_a, "rn", 1.0, name=f"dA partials {tag}")
    dx_ref = torch.where(keep, inv * (du64 @ a.double()), zero)
    dx_floor = torch.where(keep, r * SUM_EPS * inv * (du64.abs() @ a.double().abs()), zero)
    assert_rounded(dx.cpu(), dx_ref, dx_floor, f"dx {tag}")  # bound 0 where dropped: exactly zero
    assert_bits(dx.cpu()[~keep], torch.zeros(int((~keep).sum()), dtype=BF16), f"dx dropped {tag}")
