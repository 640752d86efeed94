"""csrc/skinny_gemm.hip, the bf16 form: exact bits on integer operands for every shape of the table and every K
split, placement (column blocks, padded rows, strides), NaN isolation, a row-wise bound on random data,
determinism and the refusals.  docs/TEST_TOLERANCES.md "Skinny-M GEMM" has the conditions."""
import pytest
import torch

import skinny_gemm_cases as sc
from numerics import SUM_EPS, assert_bits, assert_rounded, expect_nt, tie_share

from distributed_lion_pytorch_amd.ops import fused, hip, linear

pytestmark = pytest.mark.gpu
IDS = [f"{m}x{n}x{k}" for m, n, k in sc.CASES]


@pytest.fixture(autouse=True)
def _kernel_only(monkeypatch):
    monkeypatch.setattr(fused, "skinny_gemm_reference", lambda *a, **kw: pytest.fail("the PyTorch form ran"))


def _randn(shape, seed, device):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).to(device)


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_exact_bits_for_every_split(i, cuda):
    hip.require()
    M, N, K = sc.CASES[i]
    x, w = sc.operands(i, cuda)
    s = sc.sum64(i, cuda)
    if K >= sc.TIE_MIN_K:
        assert tie_share(s) >= sc.MIN_TIE_SHARE
    bias = sc.int_bias(i, cuda)
    plain, biased = expect_nt(s), expect_nt(s, bias)
    assert_bits(fused.skinny_gemm(x, w), plain, "default split")
    assert_bits(fused.skinny_gemm(x, w, bias), biased, "default split, bias")
    counts = sc.split_counts(i)
    assert counts[0] == 1 and len(counts) >= min(2, -(-K // 128))  # every decomposition up to what K allows
    for c in counts:
        assert_bits(fused.skinny_gemm(x, w, splits=c), plain, f"{c} splits")
        assert_bits(fused.skinny_gemm(x, w, bias, splits=c), biased, f"{c} splits, bias")


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_placement(i, cuda):
    hip.require()
    M, N, K = sc.CASES[i]
    x, w = sc.operands(i, cuda)
    exp = expect_nt(sc.sum64(i, cuda))
    counts = sc.split_counts(i)
    for c in (counts[0], counts[-1]):
        # out: a column block of a wider buffer; everything around it keeps the sentinel
        off, wide = 3, N + 11
        buf = torch.full((M + 2, wide), -77.0, dtype=torch.bfloat16, device=cuda)
        fused.skinny_gemm(x, w, out=buf[:M, off:off + N], splits=c)
        assert_bits(buf[:M, off:off + N], exp, f"column block, {c} splits")
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[:M, off:off + N] = False
        assert bool((buf[mask] == -77.0).all()), "a store outside out[:M, :N]"
        # x: rows [:M] of a 16-row buffer whose other rows are NaN, with a row stride larger than K
        xb = torch.full((16, K + 64), float("nan"), dtype=torch.bfloat16, device=cuda)
        xb[:M, :K] = x
        got = fused.skinny_gemm(xb[:M, :K], w, splits=c)
        assert bool(torch.isfinite(got).all())
        assert_bits(got, exp, f"padded, strided x, {c} splits")


@pytest.mark.parametrize("i", [1, 6, 8, 12], ids=[IDS[j] for j in (1, 6, 8, 12)])
def test_nan_and_inf_stay_in_their_row_and_column(i, cuda):
    hip.require()
    M, N, K = sc.CASES[i]
    x, w = sc.operands(i, cuda)
    clean = fused.skinny_gemm(x, w)
    m, n, k = M // 2, (2 * N) // 3, K - 3
    xn = x.clone()
    xn[m, k] = float("nan")
    got = fused.skinny_gemm(xn, w)
    rows = torch.arange(M, device=cuda) != m
    assert bool(torch.isnan(got[m]).all()) and torch.equal(got[rows], clean[rows])
    for bad in (float("nan"), float("inf")):
        wn = w.clone()
        wn[n, k] = bad
        got = fused.skinny_gemm(x, wn)
        cols = torch.arange(N, device=cuda) != n
        assert bool((~torch.isfinite(got[:, n])).all()) and torch.equal(got[:, cols], clean[:, cols])


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_random_data_within_half_an_ulp_and_the_summation_bound(i, cuda):
    hip.require()
    M, N, K = sc.CASES[i]
    x, w, bias = _randn((M, K), 600 + i, cuda), _randn((N, K), 700 + i, cuda), _randn((N,), 800 + i, cuda)
    ref = x.double() @ w.double().t() + bias.double()
    # half a bf16 ulp plus the classical bound of an fp32 sum of K terms in any order, from the reference alone
    floor = K * SUM_EPS * (x.double().abs() @ w.double().abs().t())
    a = fused.skinny_gemm(x, w, bias)
    assert_rounded(a, ref, floor, f"randn {M}x{N}x{K}")
    assert_bits(fused.skinny_gemm(x, w, bias), a, "two calls")  # determinism
    last = sc.split_counts(i)[-1]
    b = fused.skinny_gemm(x, w, bias, splits=last)
    assert_rounded(b, ref, floor, f"randn {M}x{N}x{K}, {last} splits")
    assert_bits(fused.skinny_gemm(x, w, bias, splits=last), b, "two calls, split")


@pytest.mark.parametrize("M,N,K", [(3, 4200, 640), (16, 4097, 1152)])
def test_exact_bits_unsplit_above_the_tall_form(M, N, K, cuda):
    """N > 4096 with one split: the wide form (4 row tiles per block) over several chunks, which the table's
    shapes reach only through forced splits or at K = 64."""
    hip.require()
    from numerics import exact_nt, int_operand

    x = int_operand((M, K), -7, 7, 31 + M, cuda, asym="row")
    w = int_operand((N, K), -7, 7, 41 + M, cuda, asym="col")
    s = exact_nt(x, w)
    assert tie_share(s) >= sc.MIN_TIE_SHARE
    assert fused.skinny_splits(M, N, K, 1) == (1, -(-K // 128))
    for c in (1, 2, -(-K // 128)):
        assert_bits(fused.skinny_gemm(x, w, splits=c), expect_nt(s), f"{c} splits")


def test_refusals(cuda):
    hip.require()
    w = _randn((24, 128), 1, cuda)

    def refused(x, wt, bias=None):
        assert not linear.skinny_eligible(x, wt, bias)
        with torch.no_grad():
            assert not linear.skinny_route(x, wt, bias)
        with pytest.raises(RuntimeError):
            fused.skinny_gemm(x, wt, bias)

    refused(_randn((17, 128), 2, cuda), w)  # M = 17
    refused(_randn((4, 96), 3, cuda), _randn((24, 96), 4, cuda))  # K = 96
    refused(_randn((4 * 128 + 4,), 5, cuda)[4:].view(4, 128), w)  # x 8 bytes off a 16-byte boundary
    refused(_randn((4, 132), 6, cuda)[:, :128], w)  # row stride % 8
    refused(_randn((4, 128), 7, cuda).half(), w.half())  # fp16
    refused(_randn((4, 128), 8, cuda), _randn((128, 24), 9, cuda).t())  # w not contiguous
    refused(_randn((4, 128), 10, cuda), w, _randn((24,), 11, cuda).float())  # bias dtype
    x = _randn((4, 128), 12, cuda)
    with pytest.raises(RuntimeError):  # a split count that leaves a split empty never reaches the kernel
        torch.ops.dlion.skinny_gemm_nt(x, w, None, torch.empty(4, 24, dtype=torch.bfloat16, device=cuda), 2, 1)
    with pytest.raises(RuntimeError):
        torch.ops.dlion.skinny_gemm_nt(x, w, None, torch.empty(4, 25, dtype=torch.bfloat16, device=cuda), 1, 1)
    with torch.no_grad():
        assert linear.skinny_route(x, w) and linear.skinny_route(x, w, _randn((24,), 13, cuda))
    assert not linear.skinny_route(x, w)  # gradients enabled


def test_gemm_fwd_routes_by_grad_mode(cuda, monkeypatch):
    hip.require()
    calls = []
    orig = fused.skinny_gemm
    monkeypatch.setattr(fused, "skinny_gemm", lambda *a, **kw: calls.append(a[0].shape) or orig(*a, **kw))
    x, w, b = _randn((8, 256), 20, cuda), _randn((40, 256), 21, cuda), _randn((40,), 22, cuda)
    ref = torch.nn.functional.linear(x, w, b)
    assert_bits(linear.gemm_fwd(x, w, b), ref, "grad enabled: ATen")
    assert_bits(linear.linear_nk(x, w, b), ref, "grad enabled: ATen")
    assert not calls
    with torch.no_grad():
        got = linear.gemm_fwd(x, w, b)
        assert len(calls) == 1
        got_nk = linear.linear_nk(x, w, b)
        assert len(calls) == 2
        linear.gemm_fwd(_randn((17, 256), 23, cuda), w, b)
        assert len(calls) == 2
    s = x.double() @ w.double().t() + b.double()
    floor = 256 * SUM_EPS * (x.double().abs() @ w.double().abs().t())
    assert_rounded(got, s, floor, "routed gemm_fwd")
    assert_bits(got_nk, got, "linear_nk")
    # a training step with M <= 16 rows: forward and backward stay on the parent's path
    wp = torch.nn.Parameter(w.clone())
    xg = x.clone().requires_grad_(True)
    y = linear.linear_nk(xg, wp, None)
    y.sum().backward()
    assert len(calls) == 2 and xg.grad is not None and wp.grad is not None
    monkeypatch.setattr(linear, "_SKINNY", False)  # DLION_SKINNY_GEMM=0
    with torch.no_grad():
        assert_bits(linear.gemm_fwd(x, w, b), ref, "switched off")
    assert len(calls) == 2
