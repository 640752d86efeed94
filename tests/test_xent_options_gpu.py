"""Label smoothing and z-loss in the fused LM-head cross-entropy on the GPU:
every instantiation of the options kernels against fp64 of the stored inputs,
the default path staying on the plain op, every weight-gradient route of
_LMHeadCE with the options set, and a native Llama against HF + LabelSmoother.

    loss_row = lse - (1 - eps) x_y - eps mean_{j<V}(x_j) + zeta lse^2
    grad_j   = (1 + 2 zeta lse) p_j - (1 - eps) [j == y] - eps / V
"""
import pytest
import torch
import transformers

import numerics as nm
from distributed_lion_pytorch_amd.ops import fused, hip
from test_xent_gpu import ATOL, EDGE_CASES, RTOL

pytestmark = pytest.mark.gpu

OPTIONS = [(0.1, 0.0), (0.0, 1e-3), (0.1, 1e-3)]
# + the automatic streaming choice, and the instantiations that grid does not reach: the fp32-row
# kernel at 2 and 4 vectors per thread and the 512-thread packed kernel at 16 chunks
CASES = EDGE_CASES + [(torch.bfloat16, 128256, 0), (torch.bfloat16, 12000, 1), (torch.float32, 32000, 0),
                      (torch.float16, 60000, 4)]


def _edge_rows(dtype, V, variant, cuda):
    """The rows of test_xent_gpu.test_softmax_xent_dtypes_and_edge_rows plus row 6,
    whose label logit makes p_y = 1 - 0.1: with eps = 0.1 the stored value at the
    label, (1 + 2 zeta lse) p_y - (1 - eps), is a cancellation."""
    torch.manual_seed(V + variant)
    N = 67
    Vp = 128 if V == 100 else (V + 63) // 64 * 64
    x = 2 * torch.randn(N, Vp, device=cuda)
    labels = torch.randint(0, V, (N,), device=cuda)
    labels[::7] = -100
    labels[1], labels[2], labels[3] = 0, V - 1, V - 2
    x[4, labels[4]] = x[4, :V].max() + 30
    x[5] = 10 * torch.randn(Vp, device=cuda)
    y6 = int(labels[6])
    others = torch.cat([x[6, :y6], x[6, y6 + 1:V]]).double()
    x[6, y6] = (torch.logsumexp(others, 0) + torch.log(torch.tensor(0.9 / 0.1, dtype=torch.float64))).float()
    return x.to(dtype), labels, Vp


@pytest.mark.parametrize("dtype,V,variant", CASES, ids=[f"{str(dt).split('.')[1]}-{V}-{var}" for dt, V, var in CASES])
def test_options_kernels_against_fp64(dtype, V, variant, cuda):
    """Every instantiation of launch_softmax_xent_opts on the edge rows, for three
    option pairs.  Elementwise bound RTOL |ref| + 2^-16 (1 + 2 zeta lse) p + ATOL:
    the middle term charges the fp32 error of the hardware exp and the tree sum
    (256 ulps, the model of test_xent_gpu) to the magnitude of the softmax term,
    not to the difference it cancels into."""
    hip.require()
    x, labels, Vp = _edge_rows(dtype, V, variant, cuda)
    rows = torch.arange(x.shape[0], device=cuda)
    valid = labels != -100
    safe = labels.clamp_min(0)
    x64 = x[:, :V].double()
    lse = torch.logsumexp(x64, -1)
    p = torch.exp(x64 - lse[:, None])
    assert abs(float(p[6, safe[6]]) - 0.9) < 2e-2  # row 6 is the cancellation it is meant to be
    for eps, zeta in OPTIONS:
        name = f"{dtype} V={V} variant={variant} eps={eps} zeta={zeta}"
        y = x.clone()
        loss = hip.ops().softmax_xent_opts_(y, labels, V, eps, zeta, variant)
        assert loss.dtype == torch.float32 and y.dtype == x.dtype
        soft = (1 + 2 * zeta * lse)[:, None] * p
        ref = soft - eps / V
        ref[rows, safe] -= 1 - eps
        ref[~valid] = 0
        ref_loss = (lse - (1 - eps) * x64[rows, safe] - eps * x64.mean(-1) + zeta * lse * lse) * valid
        bound = RTOL[dtype] * ref.abs() + 2.0 ** -16 * soft + ATOL
        nm.assert_within(y[:, :V], ref, bound, f"{name} gradient")
        nm.assert_elems_close(loss, ref_loss, 1e-5, 1e-5, f"{name} loss")
        assert y[~valid].abs().max().item() == 0.0, "ignored rows must be zero rows"
        assert loss[~valid].abs().max().item() == 0.0
        if Vp > V:
            assert y[:, V:].abs().max().item() == 0.0, "padded columns must store exactly 0"
        if dtype == torch.float32:
            gsum = y[:, :V].double().sum(-1)[valid]
            dev = (gsum - (2 * zeta * lse)[valid]).abs().max().item()
            print(f"[sum] {name}: max |sum_j grad_j - 2 zeta lse| {dev:.3e}")
            assert dev < 1e-4


class _OpsSpy:
    def __init__(self, real, seen):
        self._real, self._seen = real, seen

    def __getattr__(self, name):
        self._seen.append(name)
        return getattr(self._real, name)


def test_default_path_stays_on_the_plain_op(cuda, monkeypatch):
    """Options (0, 0): bit-identical loss, dh and dW to the call without the
    arguments, and the options op is never looked up."""
    hip.require()
    torch.manual_seed(11)
    V, C = 50257, 128
    h0 = torch.randn(2, 64, C, device=cuda).bfloat16()
    w0 = (0.05 * torch.randn(V, C, device=cuda)).bfloat16()
    labels = torch.randint(0, V, (2, 64), device=cuda)
    labels[0, :3] = -100
    seen = []
    real = hip.ops()
    monkeypatch.setattr(hip, "ops", lambda: _OpsSpy(real, seen))
    out = []
    for kw in ({}, {"label_smoothing": 0.0, "z_loss": 0.0}):
        h = h0.clone().requires_grad_()
        w = torch.nn.Parameter(w0.clone())
        loss = fused.lm_head_cross_entropy(h, w, labels, **kw)
        loss.backward()
        out.append((loss.detach(), h.grad, w.grad))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert "softmax_xent_" in seen and "softmax_xent_opts_" not in seen, sorted(set(seen))
    # and with an option set it is the options op that runs
    seen.clear()
    fused.lm_head_cross_entropy(h0, w0, labels, label_smoothing=0.1)
    assert "softmax_xent_opts_" in seen and "softmax_xent_" not in seen, sorted(set(seen))


EPS, ZETA = 0.1, 1e-3


def _formula(x, labels1d, eps=EPS, zeta=ZETA, normalizer=None):
    """The issue's loss from logits x [N, V] (any float dtype), by autograd-able torch ops."""
    valid = labels1d != -100
    lse = torch.logsumexp(x, -1)
    tgt = x.gather(1, labels1d.clamp_min(0)[:, None])[:, 0]
    row = lse - (1 - eps) * tgt - eps * x.mean(-1) + zeta * lse * lse
    n = valid.sum() if normalizer is None else normalizer
    return (row * valid).sum() / n


def _check_route(h, w, labels, scale, g0, name):
    """loss / h.grad / w.grad of an already-run fused call against an fp32 autograd
    reference of the formula (tolerances of tests/test_xent_gpu.py's route tests),
    and h.grad's rows against the fp64 gradient rounded to bf16."""
    V = w.shape[0]
    hr, wr = h.detach().float().requires_grad_(), w.detach().float().requires_grad_()
    ref = scale * _formula((hr @ wr.t()).view(-1, V), labels.view(-1))
    ref.backward()
    want = wr.grad + (g0.float() if g0 is not None else 0.0)
    assert (w.grad.float() - want).abs().max().item() < 2e-2 * want.abs().max().item() + 1e-4, name
    assert (h.grad.float() - hr.grad).abs().max().item() < 2e-2 * hr.grad.abs().max().item() + 1e-4, name
    h64 = h.detach().double().requires_grad_()
    (scale * _formula((h64 @ w.detach().double().t()).view(-1, V), labels.view(-1))).backward()
    nm.assert_rows_close(h.grad, h64.grad, h64.grad.bfloat16(), nm.C_ROWS, None, f"{name} h.grad")
    return ref


def test_options_wide_vocab_late_unsplit(cuda, monkeypatch):
    """Llama-3 vocabulary: the streaming options kernel, the weight gradient late
    and unsplit in the backward (shapes of test_lm_head_ce_late_unsplit_weight_grad)."""
    from distributed_lion_pytorch_amd.ops import linear

    hip.require()
    torch.manual_seed(5)
    V, C = 128256, 256
    assert linear.tn_split_factor(256, V, C, direct=True) == 1
    h = torch.randn(2, 128, C, device=cuda).bfloat16().requires_grad_()
    w = torch.nn.Parameter((0.05 * torch.randn(V, C, device=cuda)).bfloat16())
    labels = torch.randint(0, V, (2, 128), device=cuda)
    labels[0, :5] = -100
    calls = []
    late = fused._LMHeadCE._backward_late
    monkeypatch.setattr(fused._LMHeadCE, "_backward_late", staticmethod(lambda ctx, g: calls.append(1) or late(ctx, g)))
    loss = 2.5 * fused.lm_head_cross_entropy(h, w, labels, label_smoothing=EPS, z_loss=ZETA)
    loss.backward()
    assert calls == [1]
    ref = _check_route(h, w, labels, 2.5, None, "late unsplit")
    assert abs(loss.item() - ref.item()) < 2.5e-2


def test_options_gpt2_vocab_own_dgrad_gemm(cuda):
    """GPT-2 vocabulary, Parameter weight: the input gradient on the own NT GEMM
    (shapes of test_lm_head_ce_parameter_uses_own_dgrad_gemm)."""
    hip.require()
    torch.manual_seed(1)
    V, C = 50257, 128
    h = torch.randn(3, 40, C, device=cuda).bfloat16().requires_grad_()
    w = torch.nn.Parameter((0.05 * torch.randn(V, C, device=cuda)).bfloat16())
    labels = torch.randint(0, V, (3, 40), device=cuda)
    loss = fused.lm_head_cross_entropy(h, w, labels, label_smoothing=EPS, z_loss=ZETA)
    loss.backward()
    ref = _check_route(h, w, labels, 1.0, None, "own dgrad")
    assert abs(loss.item() - ref.item()) < 1e-2
    from distributed_lion_pytorch_amd.ops.linear import _WT_CACHE

    assert (id(w), "pad_t") in _WT_CACHE


@pytest.mark.parametrize("preexisting_grad", [False, True])
def test_options_weight_grad_tn_split_partials(cuda, preexisting_grad, monkeypatch):
    """Token count % 128 == 0: fp32 split partials from the own TN kernel, reduced
    + scaled (+ accumulated) in one pass, with a non-unit loss gradient (shapes of
    test_lm_head_ce_weight_grad_on_tn_kernel)."""
    hip.require()
    torch.manual_seed(3)
    V, C = 50257, 256
    h = torch.randn(2, 128, C, device=cuda).bfloat16().requires_grad_()
    w = torch.nn.Parameter((0.05 * torch.randn(V, C, device=cuda)).bfloat16())
    g0 = (0.01 * torch.randn(V, C, device=cuda)).bfloat16() if preexisting_grad else None
    if g0 is not None:
        w.grad = g0.clone()
    labels = torch.randint(0, V, (2, 128), device=cuda)
    calls = []
    parts = fused._lm_wgrad_partials
    monkeypatch.setattr(fused, "_lm_wgrad_partials", lambda *a: calls.append(1) or parts(*a))
    loss = 3.0 * fused.lm_head_cross_entropy(h, w, labels, label_smoothing=EPS, z_loss=ZETA)
    loss.backward()
    assert calls == [1]
    _check_route(h, w, labels, 3.0, g0, "TN partials")


def test_options_deferred_into_the_fusion_window(cuda, monkeypatch):
    """Two micro-batches in one fusion window (built as in test_grad_fusion_gpu):
    the head's weight gradient waits for the window's TN GEMM, and equals the sum
    of the fp32 autograd gradients of the formula, loss scales included."""
    from distributed_lion_pytorch_amd.ops import linear as L

    hip.require()
    torch.manual_seed(5)
    N, C, V = 256, 256, 1000
    hs = [torch.randn(N, C, device=cuda).bfloat16().requires_grad_(True) for _ in range(2)]
    w = torch.nn.Parameter((torch.randn(V, C, device=cuda) * 0.05).bfloat16())
    labels = [torch.randint(0, V, (N,), device=cuda) for _ in range(2)]
    labels[1][::3] = -100  # a different normalizer per micro-batch
    monkeypatch.setattr(fused, "_LM_DEFER", True)
    with L.grad_accumulation_fusion(True, micro_batches=2):
        for i in range(2):
            (fused.lm_head_cross_entropy(hs[i], w, labels[i], label_smoothing=EPS, z_loss=ZETA) * (i + 1)).backward()
            assert w.grad is None, "the deferred gradient must wait for the end of the window"
    wr = w.detach().float().requires_grad_()
    for i in range(2):
        hr = hs[i].detach().float().requires_grad_()
        ((i + 1) * _formula(hr @ wr.t(), labels[i])).backward()
        assert (hs[i].grad.float() - hr.grad).abs().max().item() < 2e-2 * hr.grad.abs().max().item() + 1e-4
        h64 = hs[i].detach().double().requires_grad_()
        ((i + 1) * _formula(h64 @ w.detach().double().t(), labels[i])).backward()
        nm.assert_rows_close(hs[i].grad, h64.grad, h64.grad.bfloat16(), nm.C_ROWS, None, f"deferred h{i}.grad")
    err = (w.grad.float() - wr.grad).abs().max().item() / wr.grad.abs().max().item()
    assert err < 2e-2, err


def test_native_llama_label_smoothing_matches_hf_smoother(cuda, tmp_path):
    """A tiny native Llama in bf16 with set_loss_options(0.1) against the stock HF
    class in fp32 (the same bf16-rounded weights) + LabelSmoother(0.1); the loss
    tolerance of tests/test_models_gpu.py."""
    from transformers.trainer_pt_utils import LabelSmoother

    from distributed_lion_pytorch_amd.models.llama import LlamaForCausalLM, llama_config

    hip.require()
    torch.manual_seed(0)
    cfg = llama_config("llama-tiny")
    ours = LlamaForCausalLM(cfg).to(torch.bfloat16)
    ours.save_pretrained(tmp_path)
    hf = transformers.LlamaForCausalLM.from_pretrained(tmp_path, torch_dtype=torch.float32).to(cuda)
    ours = ours.to(cuda)
    ours.set_loss_options(label_smoothing=0.1)
    ids = torch.randint(0, cfg.vocab_size, (4, 128), device=cuda)
    la = ours(ids, labels=ids).loss
    lb = LabelSmoother(0.1)(hf(ids), ids, shift_labels=True)
    plain = hf(ids, labels=ids).loss
    print(f"[llama] native smoothed {la.item():.5f}  HF smoother {lb.item():.5f}  HF plain {plain.item():.5f}")
    assert abs(la.item() - lb.item()) < 2e-2
    la.backward()
    assert all(torch.isfinite(p.grad).all() for p in ours.parameters() if p.grad is not None)
