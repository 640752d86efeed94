"""The fused LoRA op at the wide ranks (csrc/lora_wide.hip behind
ops/fused.lora_add): the whole op against the row-wise fp64 bounds of
lora_exact_cases.chain_bounds, the dispatch by rank, and LoRA models at r = 64
and r = 32 (over a 4-bit base) fused against unfused."""
import pytest
import torch

from distributed_lion_pytorch_amd.models.lora import LoraConfig, inject_lora
from distributed_lion_pytorch_amd.ops import fused, hip
from distributed_lion_pytorch_amd.ops import linear as L
from lora_exact_cases import chain_bounds
from lora_wide_cases import WIDE_RANKS
from numerics import assert_bits, assert_rounded

pytestmark = pytest.mark.gpu

ALL_PROJ = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]


def _rel(a, b):
    return (a.float() - b.float()).abs().max().item() / max(b.float().abs().max().item(), 1e-6)


def _spy(monkeypatch):
    calls = []
    real = fused._LoraAdd.forward
    monkeypatch.setattr(fused._LoraAdd, "forward", staticmethod(lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]))
    return calls


@pytest.mark.parametrize("r", WIDE_RANKS)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_lora_add_wide_within_chain_bounds(cuda, r, p):
    hip.require()
    torch.manual_seed(0)
    M, K, N, s = 1027, 512, 768, 2.0
    x = torch.randn(M, K, device=cuda, dtype=torch.bfloat16).requires_grad_()
    wide = torch.randn(M, 3 * N, device=cuda, dtype=torch.bfloat16)
    o = wide[:, N:2 * N].detach().requires_grad_()  # a strided column view, like a fused projection's slice
    a = (torch.randn(r, K, device=cuda) * 0.05).to(torch.bfloat16).requires_grad_()
    b = (torch.randn(N, r, device=cuda) * 0.05).to(torch.bfloat16).requires_grad_()
    seed = 1234
    out = fused._LoraAdd.apply(o, x, a, b, s, p, seed)
    dout = torch.randn(M, N, device=cuda, dtype=torch.bfloat16)
    out.backward(dout)
    # every element on its own scale: fp64 references with the two bf16 intermediates' errors propagated
    cb = chain_bounds(x, o, a, b, dout, s, p, seed)
    for name, got in (("out", out), ("dx", x.grad), ("dA", a.grad), ("dB", b.grad)):
        assert_rounded(got.detach().cpu(), cb[name][0], cb[name][1], f"lora_add {name} r={r} p={p}")
    assert_bits(o.grad, dout, "lora_add do")


def _op_case(cuda, r, M=130, K=256, N=512, s=0.5):
    g = torch.Generator().manual_seed(r)
    x = torch.randn(M, K, generator=g).to(device=cuda, dtype=torch.bfloat16).requires_grad_()
    o = torch.randn(M, N, generator=g).to(device=cuda, dtype=torch.bfloat16).requires_grad_()
    a = (torch.randn(r, K, generator=g) * 0.05).to(device=cuda, dtype=torch.bfloat16).requires_grad_()
    b = (torch.randn(N, r, generator=g) * 0.05).to(device=cuda, dtype=torch.bfloat16).requires_grad_()
    dout = torch.randn(M, N, generator=g).to(device=cuda, dtype=torch.bfloat16)
    return x, o, a, b, dout, s


def _against_fp32(x, o, a, b, dout, s):
    out = fused.lora_add(o, x, a, b, s, 0.0)
    out.backward(dout)
    xr, orf, ar, br = (t.detach().float().requires_grad_() for t in (x, o, a, b))
    ref = orf + (xr @ ar.t()) @ br.t() * s
    ref.backward(dout.float())
    assert _rel(out, ref) < 1e-2
    for got, want in ((x.grad, xr.grad), (a.grad, ar.grad), (b.grad, br.grad)):
        assert _rel(got, want) < 2e-2
    assert torch.equal(o.grad, dout)


@pytest.mark.parametrize("r", WIDE_RANKS)
def test_lora_add_reaches_the_fused_op_at_wide_ranks(cuda, monkeypatch, r):
    hip.require()
    assert r in fused.LORA_FUSED_RANKS
    calls = _spy(monkeypatch)
    _against_fp32(*_op_case(cuda, r))
    assert len(calls) == 1


@pytest.mark.parametrize("r", [4, 24, 256])
def test_lora_add_keeps_the_chain_at_other_ranks(cuda, monkeypatch, r):
    hip.require()
    assert r not in fused.LORA_FUSED_RANKS
    calls = _spy(monkeypatch)
    _against_fp32(*_op_case(cuda, r))
    assert calls == []


# ------------------------------------------------------------------ models
def _tiny_llama(cuda, r, four_bit=False):
    from distributed_lion_pytorch_amd.models.llama import LlamaForCausalLM, llama_config

    torch.manual_seed(0)
    cfg = llama_config(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                       num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=128)
    model = LlamaForCausalLM(cfg).to(device=cuda, dtype=torch.bfloat16)
    if four_bit:
        from distributed_lion_pytorch_amd.models.quant import Linear4bit, QuantConfig, quantize_model

        model = quantize_model(model, QuantConfig(bnb_4bit_compute_dtype=torch.bfloat16))
        assert isinstance(model.model.layers[0].self_attn.q_proj, Linear4bit)
    inject_lora(model, LoraConfig(r=r, lora_alpha=16, lora_dropout=0.0, target_modules=ALL_PROJ))
    for n, prm in model.named_parameters():
        if "lora_B" in n:
            torch.nn.init.normal_(prm, std=0.02)  # non-zero B so every adapter gradient is exercised
    return model


@pytest.mark.parametrize("r,four_bit", [(64, False), (32, True)], ids=["r64", "r32-4bit"])
def test_lora_llama_wide_fused_matches_unfused(cuda, monkeypatch, r, four_bit):
    """All seven projections under an adapter, inside a grad_accumulation_fusion window and under gradient
    checkpointing: loss and gradients of the fused path against the unfused chain (1e-2 on the loss, 3e-2
    relative on the gradients, the tolerances of test_lora_gpu.py)."""
    hip.require()
    model = _tiny_llama(cuda, r, four_bit)
    calls = _spy(monkeypatch)
    batches = [torch.randint(0, 512, (2, 128), device=cuda) for _ in range(2)]

    def run(flag, ckpt):
        monkeypatch.setattr(fused, "_LORA_FUSED", flag)
        if ckpt:
            model.gradient_checkpointing_enable()
        else:
            model.gradient_checkpointing_disable()
        model.zero_grad(set_to_none=True)
        n0, losses = len(calls), []
        with L.grad_accumulation_fusion(True, micro_batches=len(batches)):
            for ids in batches:
                loss = model(input_ids=ids, labels=ids).loss
                loss.backward()
                losses.append(loss.item())
        grads = {n: prm.grad.float().clone() for n, prm in model.named_parameters() if prm.grad is not None}
        return losses, grads, len(calls) - n0

    l0, g0, c0 = run(False, False)
    assert c0 == 0 and sum("lora_A" in n for n in g0) == 2 * len(ALL_PROJ)
    for ckpt in (False, True):
        l1, g1, c1 = run(True, ckpt)
        # 2 layers x 7 projections x 2 micro-batches (and again where checkpointing recomputes a layer)
        n = 2 * len(ALL_PROJ) * len(batches)
        assert c1 >= n if ckpt else c1 == n, c1
        assert all(abs(x - y) < 1e-2 for x, y in zip(l0, l1)), (l0, l1)
        assert set(g0) == set(g1)
        for n in g0:
            assert _rel(g1[n], g0[n]) < 3e-2, (n, ckpt)
