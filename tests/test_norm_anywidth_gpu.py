"""Fused residual + dropout + LayerNorm/RMSNorm at widths without an exact
instantiation (any 256 <= C <= 8192 with C % 8 == 0): the tail-predicated
kernels of csrc/norm_kernels.hip vs an fp32 PyTorch reference that uses the
identical stateless dropout mask.  Helpers and tolerances are those of
tests/test_norm_gpu.py."""
import pytest
import torch

from distributed_lion_pytorch_amd.ops import fused, hip

pytestmark = pytest.mark.gpu


def _ref(y, x, g, b, eps, p, seed, rms, bias=None):
    rows, C = x.shape
    if bias is not None:
        y = y + bias
    if p > 0:
        th = min(65535, int(round(p * 65536)))
        keep = fused.norm_dropout_keep(rows, C, p, seed, x.device)
        y = y * keep * (65536.0 / (65536.0 - th))
    xo = x + y
    if rms:
        h = xo * torch.rsqrt(xo.pow(2).mean(-1, keepdim=True) + eps) * g
    else:
        h = torch.nn.functional.layer_norm(xo, (C,), g, b, eps)
    return xo, h


def _rel(a, b):
    return (a.float() - b.float()).abs().max().item() / (b.float().abs().max().item() + 1e-6)


def _close(a, b, tol):
    """Next to the max-normalised _rel: a bound that a wrong value on a
    small-magnitude row (2-D: per-row max error / per-row max) or element
    (1-D: elementwise, atol = tolerance x the MEAN magnitude -- a column sum
    that cancels to near zero keeps the absolute rounding error of its
    summands) cannot hide under the tensor-wide maximum."""
    a, b = a.float(), b.float()
    if b.dim() >= 2:
        err = (a - b).abs().amax(-1)
        scale = b.abs().amax(-1)
        return bool((err <= tol * scale + 1e-6).all())
    return bool(((a - b).abs() <= tol * b.abs() + tol * b.abs().mean() + 1e-6).all())


# (C, rms, rows): what each width reaches in the dispatch
CASES = [
    (264, False, 333),   # smallest tail: 2 live lanes in the last chunk
    (896, True, 333),    # Qwen2-0.5B
    (1016, False, 333),  # largest one-wave tail
    (1032, True, 37),    # first multi-wave width: 2 live lanes in the third chunk
    (1280, False, 37),   # GPT-2 large
    (1600, False, 37),   # GPT-2 xl
    (3584, True, 37),    # Qwen2-7B
    (7168, True, 5),     # 7 waves per row
    (8184, False, 5),    # largest tail
    (896, True, 1),
    (3584, True, 1),
]


@pytest.mark.parametrize("C,rms,rows", CASES)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_add_norm_fwd_bwd_anywidth(C, rms, rows, p, cuda):
    hip.require()
    assert fused.norm_supported(C) and C not in fused.NORM_WIDTHS
    torch.manual_seed(0)
    x = torch.randn(rows, C, device=cuda).bfloat16()
    y = torch.randn(rows, C, device=cuda).bfloat16()
    g = (1 + 0.1 * torch.randn(C, device=cuda)).bfloat16()
    b = None if rms else (0.1 * torch.randn(C, device=cuda)).bfloat16()
    seed = 4242
    bias = (0.1 * torch.randn(C, device=cuda)).bfloat16()
    ys, xs, gs = y.clone().requires_grad_(), x.clone().requires_grad_(), g.clone().requires_grad_()
    bs = None if b is None else b.clone().requires_grad_()
    bias_s = bias.clone().requires_grad_()
    xo, h = fused._AddNorm.apply(ys, xs, bias_s, gs, bs, 1e-5, rms, p, seed)
    yr, xr, gr, bias_r = (t.float().requires_grad_() for t in (y, x, g, bias))
    br = None if b is None else b.float().requires_grad_()
    xo_r, h_r = _ref(yr, xr, gr, br, 1e-5, p, seed, rms, bias_r)
    print(f"C={C} rows={rows} p={p}: xo {_rel(xo, xo_r):.2e} h {_rel(h, h_r):.2e}")
    assert _rel(xo, xo_r) < 1e-2 and _rel(h, h_r) < 2e-2
    assert _close(xo, xo_r, 1e-2) and _close(h, h_r, 2e-2)
    dxo = torch.randn_like(x)
    dh = torch.randn_like(x)
    torch.autograd.backward([xo, h], [dxo, dh])
    torch.autograd.backward([xo_r, h_r], [dxo.float(), dh.float()])
    print(f"  dy {_rel(ys.grad, yr.grad):.2e} dx {_rel(xs.grad, xr.grad):.2e} dgamma {_rel(gs.grad, gr.grad):.2e} "
          f"dbias {_rel(bias_s.grad, bias_r.grad):.2e}")
    assert ys.grad.shape == y.shape and gs.grad.shape == (C,) and bias_s.grad.shape == (C,)
    assert _rel(ys.grad, yr.grad) < 2e-2
    assert _rel(xs.grad, xr.grad) < 2e-2
    assert _rel(gs.grad, gr.grad) < 2e-2
    assert _rel(bias_s.grad, bias_r.grad) < 2e-2
    assert _close(ys.grad, yr.grad, 2e-2) and _close(xs.grad, xr.grad, 2e-2)
    assert _close(gs.grad, gr.grad, 5e-2) and _close(bias_s.grad, bias_r.grad, 5e-2)
    if b is not None:
        assert _rel(bs.grad, br.grad) < 2e-2
        assert _close(bs.grad, br.grad, 5e-2)


@pytest.mark.parametrize("C,rms", [(896, True), (1280, False)])
def test_plain_norm_anywidth(C, rms, cuda):
    hip.require()
    torch.manual_seed(1)
    x = torch.randn(100, C, device=cuda).bfloat16().requires_grad_()
    g = (1 + 0.1 * torch.randn(C, device=cuda)).bfloat16().requires_grad_()
    b = None if rms else (0.1 * torch.randn(C, device=cuda)).bfloat16().requires_grad_()
    h = fused._Norm.apply(x, g, b, 1e-5, rms)
    xr, gr = x.detach().float().requires_grad_(), g.detach().float().requires_grad_()
    br = None if rms else b.detach().float().requires_grad_()
    hr = fused.rms_norm(xr, gr, 1e-5) if rms else torch.nn.functional.layer_norm(xr, (C,), gr, br, 1e-5)
    assert hr.dtype == torch.float32
    assert _rel(h, hr) < 2e-2 and _close(h, hr, 2e-2)
    dh = torch.randn_like(h)
    h.backward(dh)
    hr.backward(dh.float())
    assert _rel(x.grad, xr.grad) < 2e-2 and _close(x.grad, xr.grad, 2e-2)
    assert _rel(g.grad, gr.grad) < 2e-2 and _close(g.grad, gr.grad, 5e-2)
    if not rms:
        assert _rel(b.grad, br.grad) < 2e-2 and _close(b.grad, br.grad, 5e-2)


@pytest.mark.parametrize("C", [264, 1032])
@pytest.mark.parametrize("parts", [1, 7])
def test_partial_stack_sections_do_not_overlap(C, parts, cuda):
    """dh = 1, gamma = 1: the dbeta section of the [parts, 3, C] stack sums to
    exactly `rows` in every column (each block partial is a small integer, exact
    in fp32).  A masked chunk stored with the capacity's column would land in a
    neighbouring section or block and break the count."""
    hip.require()
    torch.manual_seed(2)
    rows = 37
    x = torch.randn(rows, C, device=cuda).bfloat16()
    gamma = torch.ones(C, device=cuda).bfloat16()
    beta = torch.zeros(C, device=cuda).bfloat16()
    _, _, mean, rstd = hip.ops().add_norm_fwd(x, None, None, gamma, beta, 1e-5, False, 0.0, 0)
    dh = torch.ones_like(x)
    dx, _, part = hip.ops().add_norm_bwd(dh, None, x, gamma, mean, rstd, False, 0.0, 0, False, parts)
    assert part.shape == (parts, 3, C) and dx.shape == x.shape
    assert bool(torch.isfinite(part).all())
    sums = part.sum(0)
    assert bool((sums[1] == float(rows)).all()), sums[1]
    # dgamma = sum_rows dh * xhat against the fp32 normalised rows
    xhat = (x.float() - mean[:, None]) * rstd[:, None]
    assert _rel(sums[0], xhat.sum(0)) < 2e-2
    # no branch gradient was asked for: the dbias section holds zeros
    assert bool((sums[2] == 0).all())


def test_dropout_mask_is_the_hash_at_896(cuda, monkeypatch):
    """dropout_add_norm at a tail width runs the kernel, whose keep-mask is
    norm_dropout_keep: dropped positions leave x bitwise unchanged, kept ones
    (randn inputs) almost never do -- the fp32 reference leaves 0.16-0.17 % of
    kept elements unchanged, the cap is 1 %.  The ATen composite draws an
    unrelated mask and fails the bitwise clause."""
    hip.require()
    torch.manual_seed(3)
    rows, C, p = 333, 896, 0.1
    seed = fused._new_seed()
    monkeypatch.setattr(fused, "_new_seed", lambda: seed)
    x = torch.randn(rows, C, device=cuda).bfloat16()
    y = torch.randn(rows, C, device=cuda).bfloat16()
    gamma = (1 + 0.1 * torch.randn(C, device=cuda)).bfloat16()
    xo, h = fused.dropout_add_norm(y, x, gamma, None, 1e-6, p, rms=True)
    keep = fused.norm_dropout_keep(rows, C, p, seed, cuda)
    same = xo.view(torch.int16) == x.view(torch.int16)
    assert bool(same[~keep].all())
    unchanged = same[keep].float().mean().item()
    print(f"kept positions with xo == x: {100 * unchanged:.3f} %")
    assert unchanged <= 0.01
    assert h.shape == x.shape and bool(torch.isfinite(h.float()).all())


def _rel_m(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-8)


@pytest.mark.parametrize("kind", ["qwen2", "gpt2"])
def test_models_reach_the_norm_kernel(kind, cuda, tmp_path, monkeypatch):
    """Native Qwen2 at hidden 896 and GPT-2 at hidden 320 vs the HF classes in
    bf16 (pattern and tolerances of test_models_gpu.test_native_matches_hf_on_gpu),
    with every norm of the native model routed to the fused kernel."""
    import transformers

    from distributed_lion_pytorch_amd.models import llama as L
    from distributed_lion_pytorch_amd.models.gpt2 import GPT2LMHeadModel, gpt2_config

    hip.require()
    torch.manual_seed(0)
    if kind == "gpt2":
        cfg = gpt2_config("gpt2-tiny", n_embd=320, n_head=5, n_layer=2, vocab_size=512, resid_pdrop=0.0,
                          embd_pdrop=0.0, attn_pdrop=0.0)
        ours = GPT2LMHeadModel(cfg)
        ours.save_pretrained(tmp_path)
        hf = transformers.GPT2LMHeadModel.from_pretrained(tmp_path)
        width = 320
    else:
        cfg = transformers.Qwen2Config(tie_word_embeddings=True, vocab_size=512, hidden_size=896,
                                       intermediate_size=1024, num_hidden_layers=2, num_attention_heads=14,
                                       num_key_value_heads=2, max_position_embeddings=512)
        ours = L.Qwen2ForCausalLM(cfg)
        with torch.no_grad():
            for n, p in ours.named_parameters():
                if n.endswith("proj.bias"):
                    p.normal_(0, 0.1)
        ours.save_pretrained(tmp_path)
        hf = transformers.Qwen2ForCausalLM.from_pretrained(tmp_path)
        width = 896
    ours, hf = ours.to(cuda, torch.bfloat16), hf.to(cuda, torch.bfloat16)
    routed = []
    norm_ok = fused._norm_ok

    def spy(x, gamma):
        ok = norm_ok(x, gamma)
        routed.append((x.shape[-1], ok))
        return ok

    monkeypatch.setattr(fused, "_norm_ok", spy)
    ids = torch.randint(0, cfg.vocab_size, (4, 128), device=cuda)
    la = ours(ids, labels=ids).loss
    monkeypatch.setattr(fused, "_norm_ok", norm_ok)
    # every sub-block boundary and the final norm: 2 per layer + 1
    assert len(routed) >= 2 * 2 + 1 and all(r == (width, True) for r in routed), routed
    lb = hf(ids, labels=ids).loss
    assert abs(la.item() - lb.item()) < 2e-2
    la.backward()
    lb.backward()
    for (n, p), (_, q) in zip(ours.named_parameters(), hf.named_parameters()):
        if p.grad is not None and q.grad is not None and q.grad.abs().max() > 0:
            assert _rel_m(p.grad.float(), q.grad.float()) < 0.1, n
