"""Fused softmax cross-entropy kernel (fp32-row, streaming and packed 16-bit
row variants) vs an fp32 PyTorch reference: per-row loss and the in-place
softmax - onehot."""
import re

import pytest
import torch

import numerics as nm
from distributed_lion_pytorch_amd.ops import fused, hip

pytestmark = pytest.mark.gpu

# four half-ulps of the output type.  fp32: 256 ulps for the hardware exp2 and a
# tree sum over V terms
RTOL = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -9, torch.float32: 2.0 ** -16}
ATOL = 2.0 ** -22  # one fp32 ulp of the p - 1 cancellation at the label


def _check_xent64(x, y, loss, labels, V, name):
    """y = softmax(x[:, :V]) - onehot (ignored rows and padded columns zero) and
    the per-row loss against fp64, elementwise."""
    N = x.shape[0]
    rows = torch.arange(N, device=x.device)
    valid = labels != -100
    x64 = x[:, :V].double()
    lse = torch.logsumexp(x64, -1)
    ref_loss = (lse - x64[rows, labels.clamp_min(0)]) * valid
    ref = torch.exp(x64 - lse[:, None])
    ref[rows, labels.clamp_min(0)] -= 1
    ref[~valid] = 0
    assert loss.dtype == torch.float32 and y.dtype == x.dtype
    nm.assert_elems_close(y[:, :V], ref, RTOL[x.dtype], ATOL, f"{name} softmax - onehot")
    nm.assert_elems_close(loss, ref_loss, 1e-5, 1e-5, f"{name} loss")  # exact inputs, an fp32 loss
    if x.shape[1] > V:
        assert y[:, V:].abs().max().item() == 0.0


# variant: 0 auto, 1 fp32 row in registers, 2 streaming, 4 / 5 packed row (512 / 1024 threads)
CASES = [(V, var) for V in (512, 32000, 50257) for var in (0, 1, 2, 4, 5)] + [(128256, 0), (128256, 2)]


@pytest.mark.parametrize("V,variant", CASES)
def test_softmax_xent_kernel(V, variant, cuda):
    hip.require()
    torch.manual_seed(V)
    N = 67
    Vp = (V + 63) // 64 * 64
    x = (2 * torch.randn(N, Vp, device=cuda)).bfloat16()
    labels = torch.randint(0, V, (N,), device=cuda)
    labels[::7] = -100
    ref_in = x[:, :V].float()
    y = x.clone()
    loss = hip.ops().softmax_xent_(y, labels, V, variant)
    valid = labels != -100
    ref_loss = torch.nn.functional.cross_entropy(ref_in, labels.clamp_min(0), reduction="none") * valid
    assert (loss - ref_loss).abs().max().item() < 1e-3
    prob = torch.softmax(ref_in, -1)
    prob[torch.arange(N, device=cuda), labels.clamp_min(0)] -= 1
    prob[~valid] = 0
    assert (y[:, :V].float() - prob).abs().max().item() < 1e-2
    if Vp > V:
        assert y[:, V:].abs().max().item() == 0.0
    _check_xent64(x, y, loss, labels, V, f"V={V} variant={variant}")


def _kernels_run(fn):
    """Names of the GPU kernels that fn() launches."""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return out, names


# fp32 rows have no packed kernel (variants 3..5 are 16-bit only): register-resident and streaming
EDGE_CASES = ([(dt, V, var) for dt in (torch.bfloat16, torch.float16) for V in (100, 512, 50257)
               for var in (0, 1, 2, 3, 4, 5)]
              + [(torch.float32, V, var) for V in (100, 512, 50257) for var in (0, 2)])


@pytest.mark.parametrize("dtype,V,variant", EDGE_CASES,
                         ids=[f"{str(dt).split('.')[1]}-{V}-{var}" for dt, V, var in EDGE_CASES])
def test_softmax_xent_dtypes_and_edge_rows(dtype, V, variant, cuda):
    """Every instantiation of launch_softmax_xent (bf16 / fp16 / fp32, the
    256-thread packed variant 3 included) on rows built to go wrong: labels 0,
    V-1 and V-2 (for 50257 in the last partial group of 8 before the padding),
    a label logit that dominates by 30 (p ~ 1: the stored gradient is a
    cancellation), a 10 randn row (the max subtraction), ignored rows, and
    V = 100 in 128 columns (most of a block's threads idle)."""
    hip.require()
    torch.manual_seed(V + variant)
    N = 67
    Vp = 128 if V == 100 else (V + 63) // 64 * 64
    x = 2 * torch.randn(N, Vp, device=cuda)
    labels = torch.randint(0, V, (N,), device=cuda)
    labels[::7] = -100
    labels[1], labels[2], labels[3] = 0, V - 1, V - 2
    x[4, labels[4]] = x[4, :V].max() + 30
    x[5] = 10 * torch.randn(Vp, device=cuda)
    x = x.to(dtype)
    y = x.clone()
    run = lambda: hip.ops().softmax_xent_(y, labels, V, variant)  # noqa: E731
    if variant == 3:
        # launch_packed_dt: 256 threads hold at most 25 chunks of 8 per thread
        assert (Vp + 2047) // 2048 <= 25
        loss, names = _kernels_run(run)
        assert any(re.search(r"softmax_xent_packed_kernel<\s*\d+,\s*256,", n) for n in names), names
    else:
        loss = run()
    _check_xent64(x, y, loss, labels, V, f"{dtype} V={V} variant={variant}")


def test_lm_head_ce_wide_vocab_matches_reference(cuda):
    hip.require()
    torch.manual_seed(0)
    h = torch.randn(2, 33, 64, device=cuda).bfloat16().requires_grad_()
    w = (0.05 * torch.randn(128256, 64, device=cuda)).bfloat16().requires_grad_()
    labels = torch.randint(0, 128256, (2, 33), device=cuda)
    loss = fused.lm_head_cross_entropy(h, w, labels)
    hr, wr = h.detach().float().requires_grad_(), w.detach().float().requires_grad_()
    ref = torch.nn.functional.cross_entropy((hr @ wr.t()).view(-1, 128256), labels.view(-1))
    assert abs(loss.item() - ref.item()) < 1e-2
    loss.backward()
    ref.backward()
    assert (h.grad.float() - hr.grad).abs().max().item() < 2e-2 * hr.grad.abs().max().item() + 1e-4
    # per token row against fp64; the rounding model is the fp64 gradient rounded to bf16
    h64, w64 = h.detach().double(), w.detach().double()
    logits = (h64 @ w64.t()).view(-1, 128256)
    g = torch.softmax(logits, -1)
    g[torch.arange(g.shape[0], device=cuda), labels.view(-1)] -= 1
    ref64 = ((g / g.shape[0]) @ w64).view_as(h)
    nm.assert_rows_close(h.grad, ref64, ref64.bfloat16(), nm.C_ROWS, None, "lm_head h.grad")


def test_lm_head_ce_parameter_uses_own_dgrad_gemm(cuda):
    """Parameter weight, GPT-2 vocab (padded 50304 = 393 x 128): the input
    gradient runs on the own NT GEMM against the cached padded W^T."""
    hip.require()
    torch.manual_seed(1)
    V, C = 50257, 128
    h = torch.randn(3, 40, C, device=cuda).bfloat16().requires_grad_()
    w = torch.nn.Parameter((0.05 * torch.randn(V, C, device=cuda)).bfloat16())
    labels = torch.randint(0, V, (3, 40), device=cuda)
    loss = fused.lm_head_cross_entropy(h, w, labels)
    loss.backward()
    hr, wr = h.detach().float().requires_grad_(), w.detach().float().requires_grad_()
    ref = torch.nn.functional.cross_entropy((hr @ wr.t()).view(-1, V), labels.view(-1))
    ref.backward()
    assert abs(loss.item() - ref.item()) < 1e-2
    assert (h.grad.float() - hr.grad).abs().max().item() < 2e-2 * hr.grad.abs().max().item() + 1e-4
    assert (w.grad.float() - wr.grad).abs().max().item() < 2e-2 * wr.grad.abs().max().item() + 1e-4
    from distributed_lion_pytorch_amd.ops.linear import _WT_CACHE

    assert (id(w), "pad_t") in _WT_CACHE


@pytest.mark.parametrize("preexisting_grad", [False, True])
def test_lm_head_ce_weight_grad_on_tn_kernel(cuda, preexisting_grad):
    """Token count % 128 == 0: the LM head's weight gradient comes from the own
    TN kernel as fp32 split partials, reduced + scaled (+ accumulated) in one
    pass (ops/fused._lm_wgrad_partials, sum_partials_scaled_)."""
    hip.require()
    torch.manual_seed(3)
    V, C = 50257, 256
    h = torch.randn(2, 128, C, device=cuda).bfloat16().requires_grad_()
    w = torch.nn.Parameter((0.05 * torch.randn(V, C, device=cuda)).bfloat16())
    g0 = (0.01 * torch.randn(V, C, device=cuda)).bfloat16() if preexisting_grad else None
    if g0 is not None:
        w.grad = g0.clone()
    labels = torch.randint(0, V, (2, 128), device=cuda)
    loss = 3.0 * fused.lm_head_cross_entropy(h, w, labels)  # a non-unit loss gradient
    loss.backward()
    hr, wr = h.detach().float().requires_grad_(), w.detach().float().requires_grad_()
    ref = 3.0 * torch.nn.functional.cross_entropy((hr @ wr.t()).view(-1, V), labels.view(-1))
    ref.backward()
    want = wr.grad + (g0.float() if g0 is not None else 0.0)
    assert (w.grad.float() - want).abs().max().item() < 2e-2 * want.abs().max().item() + 1e-4
    assert (h.grad.float() - hr.grad).abs().max().item() < 2e-2 * hr.grad.abs().max().item() + 1e-4


@pytest.mark.parametrize("preexisting_grad", [False, True])
def test_lm_head_ce_late_unsplit_weight_grad(cuda, preexisting_grad, monkeypatch):
    """Llama-3 vocabulary (128256, % 8 == 0) and a head the split model runs
    unsplit: the weight gradient is computed in the backward by one TN GEMM of
    the padded logits' first v columns against s * h, bf16 straight into (or
    onto) .grad (ops/fused._LMHeadCE._backward_late)."""
    from distributed_lion_pytorch_amd.ops import linear

    hip.require()
    torch.manual_seed(5)
    V, C = 128256, 256
    assert linear.tn_split_factor(256, V, C, direct=True) == 1
    h = torch.randn(2, 128, C, device=cuda).bfloat16().requires_grad_()
    w = torch.nn.Parameter((0.05 * torch.randn(V, C, device=cuda)).bfloat16())
    g0 = (0.01 * torch.randn(V, C, device=cuda)).bfloat16() if preexisting_grad else None
    if g0 is not None:
        w.grad = g0.clone()
    labels = torch.randint(0, V, (2, 128), device=cuda)
    labels[0, :5] = -100
    calls = []
    late = fused._LMHeadCE._backward_late
    monkeypatch.setattr(fused._LMHeadCE, "_backward_late", staticmethod(lambda ctx, g: calls.append(1) or late(ctx, g)))
    loss = 2.5 * fused.lm_head_cross_entropy(h, w, labels)
    loss.backward()
    assert calls == [1]
    hr, wr = h.detach().float().requires_grad_(), w.detach().float().requires_grad_()
    ref = 2.5 * torch.nn.functional.cross_entropy((hr @ wr.t()).view(-1, V), labels.view(-1))
    ref.backward()
    want = wr.grad + (g0.float() if g0 is not None else 0.0)
    assert (w.grad.float() - want).abs().max().item() < 2e-2 * want.abs().max().item() + 1e-4
    assert (h.grad.float() - hr.grad).abs().max().item() < 2e-2 * hr.grad.abs().max().item() + 1e-4
