"""CPU companion of test_elementwise_exact_gpu.py: the generators, closed forms,
exactness preconditions and tie shares of elementwise_exact_cases.py, and proof
that the case lists bite -- plain fp32 PyTorch evaluations of SwiGLU, RoPE, the
partial sums and the column sums pass every case the GPU file runs, and each
planted defect (the wrong half of the sine table in the inverse rotation, the
gate gradient without its (1 - s), a skipped row group on the two-pass route,
truncation for round-to-nearest-even) is rejected by them."""
import pytest
import torch

import elementwise_exact_cases as ec
from numerics import tie_share

LAYOUTS = ["contiguous", "halves"]
SWIGLU_CASES = [(rows, F, lay) for rows in ec.SWIGLU_ROWS for F in ec.SWIGLU_F for lay in LAYOUTS]


def _rejected(fn, *args):
    try:
        fn(*args)
    except AssertionError as e:
        return str(e).splitlines()[0]
    return None


# ------------------------------------------------------------------ SwiGLU

def test_swiglu_operands_hold_the_crafted_gates():
    for rows, F in [(257, 8), (257, 1376), (64, 64)]:
        g = ec.swiglu_operands(rows, F)[0].float()
        assert set(ec.CRAFTED) <= set(g.flatten().tolist())
    g, u, dh, buf = ec.swiglu_operands(5, 8, "halves")
    assert g.stride(0) == 24 and u.data_ptr() - g.data_ptr() == 16 and bool((buf[:, 16:] == ec.SENTINEL).all())
    # the factor 1 + g (1 - s) changes sign between the two bf16 neighbours of its zero
    g2 = torch.tensor([-1.2734375, -1.28125], dtype=torch.float64)
    f = 1 + g2 * (1 - torch.sigmoid(g2))
    assert float(f[0]) > 0 > float(f[1]) and float(f.abs().max()) < 1e-2


def test_the_reference_is_not_below_the_normal_range_at_minus_89():
    """g sigmoid(g) is 2e-37 at g = -89, sixteen times the smallest normal number, although 1 / (1 + exp(89))
    overflows to 0 in fp32; only from g = -104 on is the product itself below 2^-126."""
    g = torch.tensor([-87.0, -89.0, -200.0], dtype=torch.float64)
    s = (g * torch.sigmoid(g)).abs()
    assert float(s[0]) > float(s[1]) > 16 * ec.MIN_NORMAL and float(s[2]) < ec.MIN_NORMAL
    g32 = g.float()
    assert float((1 / (1 + torch.exp(-g32)))[1]) == 0.0 and float(ec._sigmoid32(g32)[1]) > 0.0


@pytest.mark.parametrize("rows,F,layout", SWIGLU_CASES)
def test_swiglu_fp32_evaluation_stays_inside_the_floor(rows, F, layout):
    w = ec.check_swiglu(ec.emul_swiglu(), rows, F, layout, "cpu")
    assert max(w) <= 1.0


@pytest.mark.parametrize("rows,F", ec.SWIGLU_T)
def test_swiglu_transposing_emulation(rows, F):
    ec.check_swiglu_t(ec.emul_swiglu(), rows, F, "halves", "cpu")


def test_defect_missing_one_minus_sg():
    for rows, F, layout in SWIGLU_CASES:
        assert " dg:" in _rejected(ec.check_swiglu, ec.emul_swiglu("no_one_minus_sg"), rows, F, layout, "cpu")
    for rows, F in ec.SWIGLU_T:
        assert "dgu" in _rejected(ec.check_swiglu_t, ec.emul_swiglu("no_one_minus_sg"), rows, F, "contiguous", "cpu")


# ------------------------------------------------------------------ RoPE

@pytest.mark.parametrize("H", ec.ROPE_H)
@pytest.mark.parametrize("D", ec.ROPE_D)
def test_rope_emulation_and_closed_form(H, D):
    assert ec.check_rope(ec.emul_rope(), H, D, "cpu") >= ec.MIN_TIE_SHARE
    # the closed form is the HF rotate-half definition, and its inverse the transpose: <R x, dy> == <x, R^T dy>
    x, dy, cos, sin = ec.rope_operands(H, D)
    x64, c, s = x.double(), cos.double()[None, :ec.ROPE_T, None], sin.double()[None, :ec.ROPE_T, None]
    hf = x64 * c + torch.cat([-x64[..., D // 2:], x64[..., :D // 2]], -1) * s
    assert torch.equal(ec.rope_closed(x, cos, sin, False), hf)
    lhs = (ec.rope_closed(x, cos, sin, False) * dy.double()).sum()
    rhs = (x.double() * ec.rope_closed(dy, cos, sin, True)).sum()
    assert float(lhs) == float(rhs)
    view, wide = ec.token_strided(x)
    assert view.stride(1) % 8 == 0 and view.stride(2) == D and (view.data_ptr() - wide.data_ptr()) == 16
    assert torch.equal(view, x)


@pytest.mark.parametrize("D", ec.ROPE_D)
def test_defect_wrong_sin_half(D):
    assert "inverse=True" in _rejected(ec.check_rope, ec.emul_rope("wrong_sin_half"), 5, D, "cpu")
    # tables whose halves are equal, as the HF ones are, cannot see it
    x, dy, cos, sin = ec.rope_operands(5, D)
    sym = torch.cat([sin[:, :D // 2], sin[:, :D // 2]], 1)
    assert torch.equal(ec.emul_rope("wrong_sin_half").rope(dy, cos, sym, True), ec.emul_rope().rope(dy, cos, sym, True))


# ------------------------------------------------------------------ partial sums

def test_every_route_is_hit():
    routes = {(S, n): ec.expected_route(S, n) for S, n in ec.PARTIAL_SHAPES}
    assert set(routes.values()) == {"flat", "tall", "split"}
    assert routes[(2, 2048)] == routes[(7, 7168)] == "flat" and routes[(7, 256)] == "tall"
    # at n = 16384 both sides of S = 64 / 65 are tall (n / 4 < 256 S); the switch shows at n = 65536
    assert routes[(64, 16384)] == routes[(65, 16384)] == "tall"
    assert routes[(64, 65536)] == "flat" and routes[(65, 65536)] == "tall"
    assert routes[(127, 768)] == "tall" and routes[(128, 768)] == "split" and routes[(130, 8192)] == "tall"
    # the split route with n / 4 not a multiple of 8: one and 769 float4 columns
    assert routes[(129, 4)] == routes[(1000, 3076)] == routes[(4096, 64)] == "split"
    assert [ec.split_factor(n, S) for S, n in ((129, 4), (1000, 3076), (4096, 64), (128, 768))] == [2, 6, 64, 2]
    multi = {ec.expected_route(sum(h), n, multi=True) for h, n in ec.MULTI_CASES}
    assert multi == {"multi", "split"}
    assert ec.expected_route(64, 768, multi=True) == "multi"  # [1, 33, 30]: too few rows to split


@pytest.mark.parametrize("S,n", ec.PARTIAL_SHAPES)
def test_partials_emulation(S, n):
    route, share = ec.check_partials(ec.emul_partials(), S, n, S % 2 == 1, "cpu")
    assert share >= ec.MIN_TIE_SHARE
    if route == "split":
        assert "partials" in _rejected(ec.check_partials, ec.emul_partials("skip_split_group"), S, n, False, "cpu")
    if n >= 64:  # four sums may all round down
        assert "partials" in _rejected(ec.check_partials, ec.emul_partials("trunc"), S, n, False, "cpu")


@pytest.mark.parametrize("heights,n", ec.MULTI_CASES)
def test_partials_multi_emulation(heights, n):
    route, share = ec.check_partials_multi(ec.emul_partials(), heights, n, True, "cpu")
    assert share >= ec.MIN_TIE_SHARE
    rejected = _rejected(ec.check_partials_multi, ec.emul_partials("skip_split_group"), heights, n, False, "cpu")
    # the skipped group is rows 32 .. 63 of each stack: seen on the split route where a stack is that tall
    assert (rejected is not None) == (route == "split" and max(heights) > 32)


def test_strided_stack_and_old_values():
    t = ec.partial_stack(7, 256)
    v = ec.strided_stack(t, "cpu")
    assert v.stride(0) == 768 and v.data_ptr() % 16 == 0 and torch.equal(v, t)
    old = ec.old_values(256)
    assert bool((old.float() % 8 == 0).all()) and float(old.float().abs().max()) <= 64
    exp, val = ec.partial_expected([t], "scaled4_acc", old)
    assert torch.equal(val, 4 * t.double().sum(0) + old.double()) and tie_share(val) >= ec.MIN_TIE_SHARE


# ------------------------------------------------------------------ column sums

@pytest.mark.parametrize("rows,parts", ec.COLSUM_ROWS_PARTS)
def test_colsum_emulation(rows, parts):
    for N in ec.COLSUM_N:
        assert ec.check_colsum(ec.emul_colsum, N, rows, parts, "cpu") == 0.0
    if rows > parts:
        skip = lambda x, parts: ec.emul_colsum(x[:-1], parts)  # noqa: E731 -- the last row is lost
        assert _rejected(ec.check_colsum, skip, 520, rows, parts, "cpu")


def test_defect_truncation_elementwise():
    assert _rejected(ec.check_swiglu, ec.emul_swiglu("trunc"), 257, 96, "contiguous", "cpu")
    assert _rejected(ec.check_rope, ec.emul_rope("trunc"), 5, 64, "cpu")
