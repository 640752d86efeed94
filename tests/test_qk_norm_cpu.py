"""Native Qwen3 off the GPU: parity with HF's Qwen3ForCausalLM in fp32, the
registry, the pure-PyTorch form of the per-head q/k RMSNorm + RoPE op
(fused.qk_norm_rope_reference), the FLOP / activation estimates and the
register budget of csrc/qk_norm.hip.  The bounds the GPU tests put on the
kernels are exercised here on the reference's own arithmetic."""
import tempfile

import pytest
import torch
import transformers

import numerics as nm
import qk_norm_cases as qc
from distributed_lion_pytorch_amd.models import llama as L
from distributed_lion_pytorch_amd.models import registry
from distributed_lion_pytorch_amd.ops import fused
from distributed_lion_pytorch_amd.trainer.memory import activation_bytes


def _tiny(**kw):
    """hidden 64, 4 heads on 2 kv heads, head_dim 32 != hidden / heads."""
    kw.setdefault("tie_word_embeddings", False)
    return transformers.Qwen3Config(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                                    num_attention_heads=4, num_key_value_heads=2, head_dim=32,
                                    max_position_embeddings=128, **kw)


def _randomise_gains(model):
    """Gains away from 1 (one zero, one negative per norm): a parity at the initial ones would not see them."""
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("norm.weight") or "layernorm" in n:
                p.copy_(1.0 + 0.25 * torch.randn(p.shape, generator=g))
                if "q_norm" in n or "k_norm" in n:
                    p[1], p[4] = 0.0, -0.7


def _pair(cfg):
    torch.manual_seed(0)
    ours = L.Qwen3ForCausalLM(cfg)
    _randomise_gains(ours)
    with tempfile.TemporaryDirectory() as d:
        ours.save_pretrained(d)
        hf = transformers.Qwen3ForCausalLM.from_pretrained(d)
        back = L.Qwen3ForCausalLM.from_pretrained(d)
    return ours, hf, back


def _grads_close(a, b, tol=1e-5):
    names = dict(b.named_parameters())
    n = 0
    for na, pa in a.named_parameters():
        pb = names[na]
        assert pa.grad is not None and pb.grad is not None, na
        assert torch.allclose(pa.grad, pb.grad, rtol=tol, atol=tol), (na, float((pa.grad - pb.grad).abs().max()))
        n += 1
    assert n == len(names)


@pytest.mark.parametrize("tied", [False, True])
def test_qwen3_matches_hf(tied):
    """Loss, every parameter gradient and the checkpoint round trip against the
    stock HF class (the tolerances of test_mistral_qwen2_match_hf)."""
    cfg = _tiny(tie_word_embeddings=tied)
    assert registry.NATIVE["qwen3"] is L.Qwen3ForCausalLM
    ours, hf, back = _pair(cfg)
    at = ours.model.layers[0].self_attn
    assert at.head_dim == 32 and at.q_proj.weight.shape == (128, 64) and at.k_proj.weight.shape == (64, 64)
    assert at.q_proj.bias is None and at.o_proj.bias is None
    assert at.q_norm.weight.shape == (32,) and at.k_norm.weight.shape == (32,)
    assert (ours.lm_head.weight is ours.model.embed_tokens.weight) == tied
    assert set(ours.state_dict()) == set(hf.state_dict())
    ids = torch.randint(0, cfg.vocab_size, (2, 40))
    la, lb = ours(ids, labels=ids).loss, hf(ids, labels=ids).loss
    assert abs(la.item() - lb.item()) < 1e-5, (la.item(), lb.item())
    assert abs(back(ids, labels=ids).loss.item() - la.item()) < 1e-6
    la.backward()
    lb.backward()
    _grads_close(ours, hf)
    g = at.q_norm.weight.grad
    assert g.abs().max() > 0 and g[1] != 0  # the zero gain still has a gradient
    assert [layer.self_attn.window for layer in ours.model.layers] == [0, 0]


def test_qwen3_position_ids_match_hf_per_document():
    """Documents [9, 14, 7] packed in one row with position_ids against HF run on each document alone."""
    ours, hf, _ = _pair(_tiny())
    docs = [9, 14, 7]
    T = sum(docs)
    ids = torch.randint(0, 128, (2, T))
    pos = torch.cat([torch.arange(n) for n in docs])[None].expand(2, T)
    labels = ids.clone()
    labels[pos == 0] = -100
    total, count, s = 0.0, 0, 0
    for n in docs:
        for b in range(2):
            x = ids[b:b + 1, s:s + n]
            total = total + hf(x, labels=x).loss * (n - 1)
            count += n - 1
        s += n
    lb = total / count
    la = ours(ids, labels=labels, position_ids=pos).loss
    assert abs(la.item() - lb.item()) < 1e-5, (la.item(), lb.item())
    la.backward()
    lb.backward()
    _grads_close(ours, hf)
    with pytest.raises(ValueError, match="position_ids"):  # the bounds of position_ids are checked as for Llama
        bad = pos.clone()
        bad[0, 3] = 7
        ours(ids, labels=labels, position_ids=bad)


def test_qwen3_sequence_logps_match_hf():
    """sequence_logps (DPO) against the log-softmax of HF's logits."""
    ours, hf, _ = _pair(_tiny())
    ids = torch.randint(0, 128, (3, 21))
    labels = ids.clone()
    labels[:, :5] = -100
    got = ours.sequence_logps(ids, labels)
    lp = torch.log_softmax(hf(ids).logits[:, :-1], -1)
    tgt = labels[:, 1:]
    ref = (lp.gather(-1, tgt.clamp_min(0)[..., None])[..., 0] * (tgt != -100)).sum(-1)
    assert torch.allclose(got, ref, atol=1e-4), (got, ref)


def test_qwen3_lora_adapter_sits_before_the_norm():
    """LoRA on q_proj / k_proj: merging the adapters into the base weights leaves the loss unchanged, so the
    adapter output is added to the projection before the head norm (as in HF + peft)."""
    from distributed_lion_pytorch_amd.models.lora import LoraConfig, inject_lora, merge_and_unload

    ours, hf, _ = _pair(_tiny())
    inject_lora(ours, LoraConfig(r=4, lora_alpha=8, lora_dropout=0.0, target_modules=["q_proj", "k_proj"]))
    with torch.no_grad():
        for n, p in ours.named_parameters():
            if "lora_B" in n:
                p.normal_(0, 0.2)
    ids = torch.randint(0, 128, (2, 19))
    la = ours(ids, labels=ids).loss
    la.backward()
    grads = [p.grad for n, p in ours.named_parameters() if "lora_" in n]
    assert grads and all(g is not None and g.abs().max() > 0 for g in grads)
    merged = merge_and_unload(ours)
    lm = merged(ids, labels=ids).loss
    assert abs(la.item() - lm.item()) < 1e-5
    hf.load_state_dict(merged.state_dict())
    assert abs(hf(ids, labels=ids).loss.item() - lm.item()) < 1e-5


PARAMS = {"qwen3-0.6b": 596_049_920, "qwen3-1.7b": 1_720_574_976, "qwen3-4b": 4_022_468_096,
          "qwen3-8b": 8_190_735_360}


@pytest.mark.parametrize("size", sorted(PARAMS))
def test_registry_sizes_build_on_meta(size):
    cfg = registry.load_config(size)
    assert type(cfg) is transformers.Qwen3Config and cfg.model_type == "qwen3"
    assert cfg.head_dim == 128 and cfg.num_key_value_heads == 8 and cfg.vocab_size == 151936
    assert cfg.rms_norm_eps == 1e-6 and L._rope_theta(cfg) == 1e6
    assert cfg.tie_word_embeddings == (size != "qwen3-8b")
    with torch.device("meta"):
        m = registry.build_model(cfg)
    assert type(m) is L.Qwen3ForCausalLM
    assert m.num_parameters() == PARAMS[size]  # the published counts (tied embeddings counted once)
    assert m.model.layers[0].self_attn.q_norm.weight.shape == (128,)


def test_registry_resolves_aliases_and_local_directories():
    for name, key in (("Qwen3-0.6B", "qwen3-0.6b"), ("Qwen/Qwen3-8B", "qwen3-8b"), ("Qwen3-1.7B", "qwen3-1.7b"),
                      ("Qwen3-4B", "qwen3-4b")):
        assert registry.load_config(name).to_dict() == L.llama_config(key).to_dict()
    ours = L.Qwen3ForCausalLM(_tiny())
    with tempfile.TemporaryDirectory() as d:
        ours.save_pretrained(d)
        cfg = registry.load_config(d)
        m = registry.build_model(cfg, d)
    assert type(m) is L.Qwen3ForCausalLM  # not the HF class
    assert torch.equal(m.model.layers[1].self_attn.k_norm.weight, ours.model.layers[1].self_attn.k_norm.weight)


def test_scaled_rope_raises():
    cfg = _tiny(rope_parameters={"rope_type": "yarn", "rope_theta": 1e6, "factor": 4.0,
                                 "original_max_position_embeddings": 32})
    with pytest.raises(NotImplementedError, match="yarn"):
        L.Qwen3ForCausalLM(cfg)


def test_other_families_keep_their_state_dict_keys():
    kw = dict(vocab_size=97, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
              num_key_value_heads=2, max_position_embeddings=128)
    for ours_cls, cfg_cls, hf_cls in ((L.LlamaForCausalLM, transformers.LlamaConfig, transformers.LlamaForCausalLM),
                                      (L.MistralForCausalLM, transformers.MistralConfig,
                                       transformers.MistralForCausalLM),
                                      (L.Qwen2ForCausalLM, transformers.Qwen2Config, transformers.Qwen2ForCausalLM)):
        cfg = cfg_cls(**kw)
        keys = set(ours_cls(cfg).state_dict())
        assert keys == set(hf_cls(cfg).state_dict())
        assert not any("q_norm" in k or "k_norm" in k for k in keys)


def test_reference_gradcheck():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 3, 2, 8, generator=g, dtype=torch.float64, requires_grad=True)
    gamma = (1 + 0.3 * torch.randn(8, generator=g, dtype=torch.float64)).requires_grad_()
    cos, sin = (torch.rand(5, 8, generator=g, dtype=torch.float64) * 2 - 1 for _ in range(2))
    assert torch.autograd.gradcheck(lambda a, b: fused.qk_norm_rope_reference(a, b, 1e-6, cos, sin), (x, gamma))
    assert fused.qk_norm_rope_reference(x, gamma, 1e-6, cos, sin).dtype == torch.float64
    # the public op takes the reference off the GPU and for dtypes the kernels do not cover
    got = fused.qk_norm_rope(x.detach().float(), gamma.detach().float(), 1e-6, cos.float(), sin.float())
    assert torch.allclose(got.double(), fused.qk_norm_rope_reference(x, gamma, 1e-6, cos, sin), atol=1e-5)


def test_rope_attention_with_gains_is_the_composition():
    """Off the GPU rope_attention(..., q_gamma, k_gamma) is causal_attention_gqa on the normed, rotated q / k,
    and without the gains it is what it was."""
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(2, 11, h, 16, generator=g) for h in (4, 2, 2))
    gq, gk = (1 + 0.2 * torch.randn(16, generator=g) for _ in range(2))
    cos, sin = (torch.rand(11, 16, generator=g) * 2 - 1 for _ in range(2))
    got = fused.rope_attention(q, k, v, cos, sin, q_gamma=gq, k_gamma=gk, eps=1e-6)
    ref = fused.causal_attention_gqa(fused.qk_norm_rope_reference(q, gq, 1e-6, cos, sin),
                                     fused.qk_norm_rope_reference(k, gk, 1e-6, cos, sin), v)
    assert torch.equal(got, ref)
    plain = fused.causal_attention_gqa(fused.rope(q, cos, sin), fused.rope(k, cos, sin), v)
    assert torch.equal(fused.rope_attention(q, k, v, cos, sin), plain)
    with pytest.raises(ValueError, match="pair"):
        fused.rope_attention(q, k, v, cos, sin, q_gamma=gq)


def _old_activation_bytes(config, tokens, dtype_bytes=2):
    h = getattr(config, "hidden_size", None) or getattr(config, "n_embd")
    ff = getattr(config, "intermediate_size", None) or getattr(config, "n_inner", None) or 4 * h
    layers = getattr(config, "num_hidden_layers", None) or getattr(config, "n_layer")
    return tokens * (layers * (6 * h + 4 * ff) * dtype_bytes + 4 * getattr(config, "vocab_size", 0))


@pytest.mark.parametrize("name", ["llama-2-7b", "llama-3-8b", "mistral-7b", "qwen2-0.5b", "gpt2", "qwen3-0.6b"])
def test_estimates(name):
    """activation_bytes and flops_per_token count the attention width heads x head_dim: unchanged where that is
    the hidden size (every family before Qwen3), larger for Qwen3-0.6B (2048 against 1024, plus the kept
    pre-norm q | k block and rstd)."""
    cfg = registry.load_config(name)
    with torch.device("meta"):
        m = registry.build_model(cfg)
    new_act, old_act = activation_bytes(cfg, 4096), _old_activation_bytes(cfg, 4096)
    if name == "gpt2":
        assert new_act == old_act
        return
    T = 1024
    old_flops = 6 * m.num_parameters() + 12 * cfg.num_hidden_layers * cfg.hidden_size * T
    if name == "qwen3-0.6b":
        assert new_act > old_act and m.flops_per_token(T) > old_flops
        assert m.flops_per_token(T) == 6 * m.num_parameters() + 12 * 28 * 2048 * T
        assert new_act - old_act == 4096 * 28 * (3 * 1024 * 2 + 24 * 128 * 2 + 24 * 4)
    else:
        assert new_act == old_act and m.flops_per_token(T) == old_flops


@pytest.mark.parametrize("T,H,Hkv,D", [s for s in qc.SHAPES if s[0] in (1, 33)])
def test_bounds_hold_for_the_reference_arithmetic(T, H, Hkv, D):
    """The GPU tests' bounds on these very inputs: the fp32 PyTorch form and a second fp32 realisation with another
    summation order (emulate_fwd32: a lane per 8 dims) pass assert_rounded with the per-row floor once rounded to
    bf16, the second one's rstd is within 4 x 2^-24, and the fp32 form's dx passes its floor."""
    x, dz, gq, gk, cos, sin = qc.inputs(T, H, Hkv, D)
    z64, dx64, _, _ = qc.form(x, gq, gk, H, cos, sin, dz, torch.float64)
    z32, dx32, _, _ = qc.form(x, gq, gk, H, cos, sin, dz, torch.float32)
    floor = qc.row_floor(z32, z64)
    assert float(floor[0, 0, 0].max()) == 0.0 and bool((z64[0, 0, 0] == 0).all())  # the all-zero head row
    nm.assert_rounded(z32.to(torch.bfloat16), z64, floor, "fp32 form")
    z2, r2 = qc.emulate_fwd32(x, gq, gk, H, cos, sin)
    used = nm.assert_rounded(z2.to(torch.bfloat16), z64, floor, "second fp32 realisation")
    assert used <= 1.0
    _, r64 = qc.stats64(x)
    assert float(r64[0, 0, 0]) == pytest.approx(1e3)
    ratio = ((r2.double() - r64).abs() / (4 * 2.0 ** -24 * r64)).max()
    assert float(ratio) <= 1.0, float(ratio)
    nm.assert_rounded(dx32.to(torch.bfloat16), dx64, qc.row_floor(dx32, dx64), "fp32 form dx")


def test_kernels_do_not_spill(tmp_path):
    from test_kernel_resources_cpu import _resources

    res = {k: v for k, v in _resources("qk_norm.hip", [], tmp_path).items() if "qk_norm_rope" in k}
    assert len(res) == 6, sorted(res)  # fwd x {64, 128}, bwd x {64, 128} x {dz with tables, dy}
    for name, r in res.items():
        assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        print(name, r)
