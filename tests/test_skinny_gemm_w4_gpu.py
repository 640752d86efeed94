"""csrc/skinny_gemm.hip, the 4-bit form: bit-identity with the bf16 form on the dequantised weight (both real
codebooks, an all-zero block and a huge scale included), exact bits on an integer codebook (the case whose CPU twin
rejects a swapped nibble order and a misplaced scale), and Linear4bit's routing: a decode step expands nothing."""
import pytest
import torch

import skinny_gemm_cases as sc
from numerics import assert_bits, exact_nt, expect_nt, tie_share

from distributed_lion_pytorch_amd.models import quant as mq
from distributed_lion_pytorch_amd.ops import fused, hip, quant

pytestmark = pytest.mark.gpu
IDS = [f"{m}x{n}x{k}" for m, n, k in sc.CASES]


@pytest.fixture(autouse=True)
def _kernel_only(monkeypatch):
    monkeypatch.setattr(fused, "skinny_gemm_reference", lambda *a, **kw: pytest.fail("the PyTorch form ran"))
    monkeypatch.setattr(fused, "skinny_gemm_w4_reference", lambda *a, **kw: pytest.fail("the PyTorch form ran"))


def _randn(shape, seed, device):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).to(device)


@pytest.mark.parametrize("name", ["nf4", "fp4"])
@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_identical_to_the_bf16_kernel_on_the_dequantised_weight(i, name, cuda):
    hip.require()
    M, N, K = sc.CASES[i]
    assert (N * K) % 64 == 0
    code = quant.code_tensor(name, cuda)
    x, w, bias = _randn((M, K), 900 + i, cuda), _randn((N, K), 1000 + i, cuda), _randn((N,), 1100 + i, cuda)
    q, a = quant.quantize_4bit(w, code)
    nb = a.numel()
    a[nb // 2] = 0.0  # an all-zero block
    a[nb - 1] = 2.0 ** 100  # a huge scale (products and sums stay finite)
    wd = quant.dequantize_4bit(q, a, code, (N, K))
    assert wd.dtype == torch.bfloat16 and bool(torch.isfinite(wd).all())
    assert bool((wd.view(-1, 64)[nb // 2] == 0).all()) and float(wd.view(-1, 64)[nb - 1].abs().max()) >= 2.0 ** 98
    counts = sc.split_counts(i)
    for c in (None, counts[-1]):
        assert_bits(fused.skinny_gemm_w4(x, q, a, code, N, splits=c), fused.skinny_gemm(x, wd, splits=c), f"{name} {c}")
        assert_bits(fused.skinny_gemm_w4(x, q, a, code, N, bias, splits=c), fused.skinny_gemm(x, wd, bias, splits=c),
                    f"{name} {c} bias")


@pytest.mark.parametrize("i", sc.W4_EXACT, ids=[IDS[j] for j in sc.W4_EXACT])
def test_exact_bits_on_an_integer_codebook(i, cuda):
    hip.require()
    M, N, K = sc.CASES[i]
    x, q, a, code = sc.w4_exact(i, cuda)
    s = exact_nt(x, sc.w4_values(q, a, code, N, K))
    if K >= 256:
        assert tie_share(s) >= sc.MIN_TIE_SHARE
    exp = expect_nt(s)
    for c in sc.split_counts(i):
        assert_bits(fused.skinny_gemm_w4(x, q, a, code, N, splits=c), exp, f"{c} splits")
    buf = torch.full((M, N + 9), 5.0, dtype=torch.bfloat16, device=cuda)
    fused.skinny_gemm_w4(x, q, a, code, N, out=buf[:, 4:4 + N])
    assert_bits(buf[:, 4:4 + N], exp, "column block")
    assert bool((buf[:, :4] == 5).all()) and bool((buf[:, 4 + N:] == 5).all())


def test_refusals(cuda):
    hip.require()
    code = quant.code_tensor("nf4", cuda)
    q, a = quant.quantize_4bit(_randn((24, 128), 1, cuda), code)
    x = _randn((4, 128), 2, cuda)
    fused.skinny_gemm_w4(x, q, a, code, 24)
    with pytest.raises(RuntimeError):
        fused.skinny_gemm_w4(_randn((17, 128), 3, cuda), q, a, code, 24)
    with pytest.raises(RuntimeError):
        fused.skinny_gemm_w4(x.half(), q, a, code, 24)
    with pytest.raises(RuntimeError):
        fused.skinny_gemm_w4(x, q, a[:-1], code, 24)
    with pytest.raises(RuntimeError):
        fused.skinny_gemm_w4(x, q, a, code[:8], 24)
    with pytest.raises(ValueError):
        fused.skinny_gemm_w4(x, q, a, code, 25)


def test_linear4bit_routing(cuda, monkeypatch):
    hip.require()
    torch.manual_seed(0)
    K = 256
    lins = [torch.nn.Linear(K, n, bias=False, device=cuda, dtype=torch.bfloat16) for n in (256, 64)]
    layers = [mq.Linear4bit.from_linear(l, "nf4") for l in lins]
    x = _randn((2, 4, K), 5, cuda)  # [B, 4, K]: 8 rows
    expanded = []
    orig = mq.dequantize_4bit
    monkeypatch.setattr(mq, "dequantize_4bit", lambda *a, **kw: expanded.append(1) or orig(*a, **kw))
    # gradients enabled: the expansion path, as before
    ya = mq.linear4bit_multi(x, layers)
    assert len(expanded) == 2 and [tuple(y.shape) for y in ya] == [(2, 4, 256), (2, 4, 64)]
    # a decode step: nothing may be expanded
    monkeypatch.setattr(mq, "dequantize_4bit", lambda *a, **kw: pytest.fail("a 4-bit weight was expanded"))
    monkeypatch.setattr(torch.ops.dlion, "dequant4_", lambda *a, **kw: pytest.fail("dequant4_ ran"), raising=False)
    monkeypatch.setattr(torch.ops.dlion, "dequant4_t_", lambda *a, **kw: pytest.fail("dequant4_t_ ran"), raising=False)
    x2d = x.reshape(-1, K)
    with torch.no_grad():
        yb = mq.linear4bit_multi(x, layers)
        for l, y in zip(layers, yb):
            assert_bits(y.reshape(8, -1), fused.skinny_gemm_w4(x2d, l.qweight, l.absmax, l.quant_map, l.out_features),
                        "per-layer kernel")
        # the outputs are column blocks of one buffer, as the expansion path's single GEMM returns them
        assert yb[1].data_ptr() == yb[0].data_ptr() + 256 * 2
        # one layer with a bias
        lb = mq.Linear4bit.from_linear(torch.nn.Linear(K, 72, bias=True, device=cuda, dtype=torch.bfloat16), "fp4")
        assert_bits(lb(x).reshape(8, -1),
                    fused.skinny_gemm_w4(x2d, lb.qweight, lb.absmax, lb.quant_map, 72, lb.bias), "bias")
    # the two paths compute the same product: they agree to bf16 rounding of the same fp32-accumulated sums
    for a_, b_ in zip(ya, yb):
        assert float((a_.float() - b_.float()).abs().max()) <= 2.0 ** -7 * float(a_.float().abs().max())
