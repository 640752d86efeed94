"""The exact-GEMM helpers of tests/numerics.py without a GPU: the generators
meet the conditions test_gemm_exact_gpu.py relies on at every shape it uses,
the fp64 closed forms equal fp64 autograd of F.gelu, and the checkers reject
planted wrong answers (and accept the correctly rounded ones)."""
import pytest
import torch
import torch.nn.functional as F

from gemm_exact_cases import (EDGE_SHAPES, GELU_SCALE, MIN_TIE_SHARE, NT_SHAPES, TN_CASES, nt_operands, tn_operands,
                              tn_split_rows)
from numerics import (EVAL_MARGIN, GEMM_SLAB, assert_bits, assert_col_partials, assert_rounded, bf16_half_ulp,
                      eval_floor, exact_nt, exact_tn, expect_nt, gelu64, gelu_form, gelu_grad64, gelu_grad_form,
                      gemm_slabs, int_operand, strided_rows, tie_share)

BF16 = torch.bfloat16


def _truncate(x64):
    """fp64 -> bf16 by dropping the low 16 bits of the fp32 value (round toward zero)."""
    bits = x64.float().contiguous().view(torch.int32)
    return (bits & ~0xFFFF).view(torch.float32).to(BF16)


# --------------------------------------------------------------------------- generators
def test_tie_share_counts_exactly_the_ties():
    x = torch.tensor([255.0, 256.0, 257.0, 258.0, 259.0, 511.0, 512.0, 513.0, 514.0, 516.0, 518.0, 1028.0, 1032.0, 0.0, -257.0,
                      257.0 / 64, 258.0 / 64], dtype=torch.float64)
    ties = torch.tensor([0, 0, 1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0], dtype=torch.bool)
    for v, t in zip(x.tolist(), ties.tolist()):
        assert (tie_share(torch.tensor([v], dtype=torch.float64)) == 1.0) == t, v
        # a tie is exactly where round-to-nearest-even and round-half-away differ or rounding is not exact
        assert (float(torch.tensor(v).to(BF16)) != v) >= t
    assert tie_share(x) == float(ties.double().mean())


@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_nt_cases_are_exact_and_full_of_ties(M, N, K):
    scales = (1.0, GELU_SCALE) if (M, N, K) in EDGE_SHAPES else (1.0,)
    for scale in scales:
        a, b = nt_operands(M, N, K, "cpu", scale)
        s = exact_nt(a, b)  # asserts max sum |a b| < 2^24
        assert tie_share(s) >= MIN_TIE_SHARE, (M, N, K, scale, tie_share(s))
        assert torch.equal(s.float().double(), s)
        # asymmetric: the transposed problem is another matrix
        if M == N:
            assert not torch.equal(s, s.t())


@pytest.mark.parametrize("M,N,rows,nseg,splits,ldp_pad,ldq_pad", TN_CASES)
def test_tn_cases_are_exact_and_full_of_ties(M, N, rows, nseg, splits, ldp_pad, ldq_pad):
    P, Q = tn_operands(M, N, rows, nseg, "cpu")
    s = exact_tn(P, Q)
    assert tie_share(s) >= MIN_TIE_SHARE, tie_share(s)
    Pc, Qc = torch.cat(P), torch.cat(Q)
    spans = tn_split_rows(rows, nseg, splits)
    assert spans[0][0] == 0 and spans[-1][1] == rows * nseg
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and all(r1 > r0 for r0, r1 in spans)
    assert torch.equal(sum(exact_tn(Pc[r0:r1], Qc[r0:r1]) for r0, r1 in spans), s)


def test_exactness_condition_is_asserted_not_assumed():
    a = int_operand((8, 128), 200, 255, 0, "cpu", asym=None)
    b = int_operand((8, 128), 200, 255, 1, "cpu", asym=None)
    exact_nt(a, b)  # 128 * 255^2 < 2^24
    big = torch.cat([a] * 4, 1), torch.cat([b] * 4, 1)  # 512 * 200^2 > 2^24
    with pytest.raises(AssertionError, match="not exact"):
        exact_nt(*big)
    with pytest.raises(AssertionError, match="not exact"):
        exact_tn(big[0].t().contiguous(), big[1].t().contiguous())


# --------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("exact", [False, True])
def test_closed_forms_equal_fp64_autograd(exact):
    u = torch.linspace(-12, 12, 48001, dtype=torch.float64).requires_grad_(True)
    y = F.gelu(u, approximate="none" if exact else "tanh")
    y.backward(torch.ones_like(y))
    assert (gelu64(u, exact) - y.detach()).abs().max() < 1e-14
    assert (gelu_grad64(u, exact) - u.grad).abs().max() < 1e-14


@pytest.mark.parametrize("exact", [False, True])
def test_eval_floor_is_far_below_half_an_ulp(exact):
    g = torch.Generator().manual_seed(5)
    u = (torch.rand(200000, generator=g) * 24 - 12).to(BF16).float()
    for fn in (gelu_form, gelu_grad_form):
        fl = eval_floor(lambda t: fn(t, exact), u)
        print(f"eval_floor {fn.__name__} exact={exact}: {fl / EVAL_MARGIN * 2 ** 24:.2f} x 2^-24 before the margin")
        assert 0 < fl < 2.0 ** -9 / 64


# --------------------------------------------------------------------------- assert_rounded
def _values(n=20000, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * torch.exp(3 * torch.randn(n, generator=g))).double()


def test_assert_rounded_accepts_the_correct_rounding_and_only_that():
    ref = torch.cat([_values(), torch.tensor([257.0, 259.0, 1.00390625, 0.0, -514.0], dtype=torch.float64)])
    good = ref.to(BF16)
    assert assert_rounded(good, ref, 0.0, "rne") == 1.0  # the planted ties sit exactly on the bound
    # the flat 2^-9 |ref| is NOT half an ulp at the bottom of a binade: it rejects bf16(ref) itself
    err = (good.double() - ref).abs()
    assert float((err / (2.0 ** -9 * ref.abs()).clamp_min(1e-300)).max()) > 1.9
    assert bool((bf16_half_ulp(ref) >= 2.0 ** -9 * ref.abs()).all()) and bool((bf16_half_ulp(ref) <= 2.0 ** -8 * ref.abs()).all())
    # truncation instead of rounding
    with pytest.raises(AssertionError, match="over half a bf16 ulp"):
        assert_rounded(_truncate(ref), ref, 0.0, "truncated")
    # rounding ties away from zero instead of to even: only the exact ties differ
    away = good.clone()
    away[-5], away[-1] = 258.0, -516.0
    with pytest.raises(AssertionError):
        assert_bits(away, good, "ties away")
    # one ulp off in a single element
    off = good.clone()
    off[7] = (good[7].float() * (1 + 2.0 ** -7)).to(BF16)
    assert off[7] != good[7]
    with pytest.raises(AssertionError):
        assert_rounded(off, ref, 0.0, "one ulp")
    with pytest.raises(AssertionError, match="non-finite"):
        assert_rounded(torch.full_like(good, float("nan")), ref, 0.0, "nan")


@pytest.mark.parametrize("exact", [False, True])
def test_gelu_checks_reject_truncation_and_a_shifted_bias(exact):
    M, N, K = 129, 264, 256
    a, b = nt_operands(M, N, K, "cpu", GELU_SCALE)
    s = exact_nt(a, b)
    g = torch.Generator().manual_seed(9)
    bias = torch.randn(N, generator=g).to(BF16)
    z = expect_nt(s)
    u = z.float() + bias.float()
    for form in (gelu_form, gelu_grad_form):
        fn = lambda t: form(t, exact)  # noqa: E731
        ref, fl = fn(u.double()), eval_floor(fn, u)
        assert assert_rounded(fn(u).to(BF16), ref, fl, "fp32 evaluation") <= 1.0
        with pytest.raises(AssertionError):
            assert_rounded(_truncate(ref), ref, fl, "truncated")
        shifted = z.float() + torch.roll(bias, 1).float()
        with pytest.raises(AssertionError):
            assert_rounded(fn(shifted).to(BF16), ref, fl, "bias shifted by one column")
    # the bit-exact bias epilogue
    with pytest.raises(AssertionError):
        assert_bits(expect_nt(s, torch.roll(bias, 1)), expect_nt(s, bias), "bias shifted by one column")
    with pytest.raises(AssertionError):
        assert_bits(_truncate(s), expect_nt(s), "truncated")
    assert_bits(expect_nt(s, bias), (s.float() + bias.float()).to(BF16), "bias")


# --------------------------------------------------------------------------- partials
def _wave_partials(dz, row_sets):
    """What the kernels compute: an fp32 running sum of the stored bf16 values per row set."""
    out = torch.zeros(len(row_sets), dz.shape[1])
    for s, rows in enumerate(row_sets):
        for row in dz[rows].float():
            out[s] += row
    return out


@pytest.mark.parametrize("integer", [True, False])
def test_partials_checker_rejects_planted_defects(integer):
    M, N = 300, 72  # 3 slabs with rows, the 4th empty
    g = torch.Generator().manual_seed(2)
    if integer:
        dz = torch.randint(-3000, 3001, (M, N), generator=g).float().to(BF16)
    else:
        dz = (torch.randn(M, N, generator=g) * 50).to(BF16)
    slabs = gemm_slabs(M)
    assert [(s.start, s.stop) for s in slabs] == [(0, 128), (128, 256), (256, 300), (300, 300)]
    part = _wave_partials(dz, slabs)

    def check(p, name):
        return assert_col_partials(p, dz, slabs, GEMM_SLAB, exact=integer, name=name)

    assert check(part, "correct") <= 1.0
    assert bool((part[3] == 0).all())
    # one row dropped from a slab
    dropped = part.clone()
    dropped[1] -= dz[200].float()
    with pytest.raises(AssertionError, match="partial row 1"):
        check(dropped, "row dropped")
    # two slabs swapped (what part[2 tm + (wr ^ 1)] does)
    with pytest.raises(AssertionError):
        check(part[[1, 0, 3, 2]], "slabs swapped")
    with pytest.raises(AssertionError):
        check(part[[0, 1, 3, 2]], "last slabs swapped")
    # an empty slab that is not zero, a wrong shape, the sum of the unrounded values
    dirty = part.clone()
    dirty[3, 5] = 1e-30
    with pytest.raises(AssertionError, match="not zero"):
        check(dirty, "dirty empty slab")
    with pytest.raises(AssertionError, match="shape"):
        check(part[:3], "short")
    if not integer:
        unrounded = _wave_partials((dz.float() * (1 + 2.0 ** -10)), slabs)
        with pytest.raises(AssertionError):
            check(unrounded, "sum of unrounded products")


def test_strided_row_sets_and_their_empty_blocks():
    rows, N = 5, 16
    g = torch.Generator().manual_seed(4)
    dz = torch.randn(rows, N, generator=g).to(BF16)
    sets = strided_rows(rows, rows + 3)
    assert [len(s) for s in sets] == [1] * 5 + [0] * 3
    part = _wave_partials(dz, sets)
    assert_col_partials(part, dz, sets, name="one row per block")
    bad = part.clone()
    bad[6, 0] = 1.0
    with pytest.raises(AssertionError, match="not zero"):
        assert_col_partials(bad, dz, sets, name="dirty")
    sets7 = strided_rows(300, 7)
    assert sorted(torch.cat(sets7).tolist()) == list(range(300))
