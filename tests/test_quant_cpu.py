"""4-bit frozen bases (models/quant.py, ops/quant.py) on the CPU: the
quantization contract (64-element blocks, fp32 absmax, nearest codebook
entry, first element in the high nibble), Linear4bit == nn.Linear over the
dequantized weight, QLoRA training through the fused Llama projections, LoRA
merge into a 4-bit base, and the ``--load_in_4bit`` entrypoints.

Reference: bitsandbytes 4-bit NF4 bases of /root/reference/sft_llama2.py:141-154
and dpo_llama2.py:133-152.  bitsandbytes is not installed, so byte-level parity
with its checkpoints is unpinned; the codebooks are its published tables."""
import os

import pytest
import torch
import torch.nn as nn

from distributed_lion_pytorch_amd.models.llama import LlamaForCausalLM, llama_config
from distributed_lion_pytorch_amd.models.lora import LoraConfig, LoraLinear, inject_lora, merge_and_unload
from distributed_lion_pytorch_amd.models.quant import (Linear4bit, QuantConfig, dequantize_model, quantize_model,
                                                       quantized_bytes)
from distributed_lion_pytorch_amd.ops.quant import (NF4_CODE, code_tensor, dequantize_4bit, dequantize_4bit_ref,
                                                    quantize_4bit, quantize_4bit_ref)
from numerics import assert_bits
from quant_edge_cases import (DEQUANT_WORDS, DTYPES, EDGE_ABSMAX, crafted_blocks, edge_packed, random_packed,
                              tie_points)


@pytest.mark.parametrize("qt", ["nf4", "fp4"])
def test_quantize_contract(qt):
    torch.manual_seed(0)
    w = torch.randn(96, 128)
    code = code_tensor(qt)
    q, absmax = quantize_4bit(w, code)
    assert q.dtype == torch.uint8 and q.numel() == w.numel() // 2
    assert torch.equal(absmax, w.reshape(-1, 64).abs().amax(1))
    idx = torch.stack([q >> 4, q & 15], 1).reshape(-1, 64).long()  # high nibble first
    x = w.reshape(-1, 64) / absmax[:, None]
    # every element maps to a nearest codebook entry
    err = (x - code[idx]).abs()
    best = (x.unsqueeze(-1) - code).abs().amin(-1)
    assert torch.equal(err, best)
    d = dequantize_4bit(q, absmax, code, w.shape, torch.float32)
    assert torch.equal(d, (code[idx] * absmax[:, None]).reshape(w.shape))
    rel = ((d - w).norm() / w.norm()).item()
    assert rel < (0.11 if qt == "nf4" else 0.14)
    # the block max is represented exactly (code has +-1)
    assert torch.allclose(d.reshape(-1, 64).abs().amax(1), absmax)


def test_zero_block_and_nf4_table():
    assert len(NF4_CODE) == 16 and NF4_CODE[7] == 0.0 and NF4_CODE[0] == -1.0 and NF4_CODE[15] == 1.0
    w = torch.zeros(2, 64)
    w[1, 5] = 3.0
    q, a = quantize_4bit_ref(w, code_tensor("nf4"))
    assert a[0] == 0 and a[1] == 3.0
    d = dequantize_4bit_ref(q, a, code_tensor("nf4"), torch.float32).view(2, 64)
    assert torch.equal(d, w)


def test_linear4bit_matches_dequantized_linear():
    torch.manual_seed(0)
    lin = nn.Linear(128, 192, bias=True)
    q4 = Linear4bit.from_linear(lin, "nf4")
    ref = nn.Linear(128, 192, bias=True)
    with torch.no_grad():
        ref.weight.copy_(q4.dequantize(torch.float32))
        ref.bias.copy_(lin.bias)
    x = torch.randn(5, 7, 128, requires_grad=True)
    xr = x.detach().clone().requires_grad_()
    y = q4(x)
    yr = ref(xr)
    assert torch.allclose(y, yr, atol=1e-5)
    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g)
    assert torch.allclose(x.grad, xr.grad, atol=1e-5)
    assert all(not p.requires_grad for p in q4.parameters())
    # state_dict round trip
    q4b = Linear4bit(128, 192, bias=True, compute_dtype=torch.float32)
    q4b.load_state_dict(q4.state_dict())
    assert torch.equal(q4b.dequantize(), q4.dequantize())


def _tiny(seed=0):
    torch.manual_seed(seed)
    return LlamaForCausalLM(llama_config("llama-tiny"))


def test_qlora_equals_lora_on_dequantized_base():
    """A 4-bit base + LoRA computes the same loss and adapter gradients as
    bf16/fp32 LoRA on the dequantized weights (fused q/k/v, gate/up path)."""
    m4 = quantize_model(_tiny(), QuantConfig())
    assert isinstance(m4.model.layers[0].mlp.gate_proj, Linear4bit)
    assert type(m4.lm_head) is nn.Linear  # skipped like bitsandbytes
    mr = dequantize_model(quantize_model(_tiny(), QuantConfig()))
    assert type(mr.model.layers[0].mlp.gate_proj) is nn.Linear
    cfg = LoraConfig(r=8, lora_alpha=16, lora_dropout=0.0, target_modules=["q_proj", "v_proj", "up_proj"])
    torch.manual_seed(1)
    inject_lora(m4, cfg)
    torch.manual_seed(1)
    inject_lora(mr, cfg)
    pr_by_name = dict(mr.named_parameters())
    for n, p in m4.named_parameters():
        if "lora_" in n:
            with torch.no_grad():
                if "lora_B" in n:
                    p.normal_(0, 0.02)
                pr_by_name[n].copy_(p)
    ids = torch.randint(0, 512, (2, 64))
    l4 = m4(input_ids=ids, labels=ids).loss
    lr = mr(input_ids=ids, labels=ids).loss
    assert torch.allclose(l4, lr, atol=1e-5)
    l4.backward()
    lr.backward()
    g4 = {n: p.grad for n, p in m4.named_parameters() if p.requires_grad}
    gr = {n: p.grad for n, p in mr.named_parameters() if p.requires_grad}
    assert set(g4) == set(gr) and len(g4) == 12
    for n in g4:
        assert torch.allclose(g4[n], gr[n], atol=1e-5, rtol=1e-4), n


def test_qlora_merge_and_memory():
    m = quantize_model(_tiny(), QuantConfig())
    n_lin = sum(l.in_features * l.out_features for l in m.modules() if isinstance(l, Linear4bit))
    assert quantized_bytes(m) < 0.6 * n_lin  # ~0.5625 B/param
    inject_lora(m, LoraConfig(r=8, lora_alpha=16, lora_dropout=0.0))
    lora = m.model.layers[0].self_attn.q_proj
    assert isinstance(lora, LoraLinear) and isinstance(lora.base_layer, Linear4bit)
    with torch.no_grad():
        lora.lora_B.weight.normal_(0, 0.05)
    ids = torch.randint(0, 512, (1, 64))
    before = m(input_ids=ids, labels=ids).loss
    merged = merge_and_unload(dequantize_model(m))
    assert type(merged.model.layers[0].self_attn.q_proj) is nn.Linear
    after = merged(input_ids=ids, labels=ids).loss
    assert torch.allclose(before, after, atol=1e-4)


def test_sft_dpo_entrypoints_load_in_4bit(tmp_path):
    import dpo_llama2
    import sft_llama2

    sft_out = str(tmp_path / "sft")
    sft_llama2.main(["--model_name", "llama-tiny", "--synthetic_data", "--synthetic_samples", "100", "--seq_length", "64",
                     "--output_dir", sft_out, "--max_steps", "2", "--per_device_train_batch_size", "2",
                     "--learning_rate", "1e-3", "--lion", "--async_grad", "--report_to", "none", "--use_cpu",
                     "--torch_dtype", "float32", "--load_in_4bit", "--save_strategy", "no"])
    merged = os.path.join(sft_out, "final_merged_checkpoint")
    assert os.path.isfile(os.path.join(sft_out, "final_checkpoint", "adapter_model.safetensors"))
    from safetensors.torch import load_file

    sd = load_file(os.path.join(merged, "model.safetensors"))
    assert "model.layers.0.self_attn.q_proj.weight" in sd and not any("qweight" in k for k in sd)
    tr = dpo_llama2.main(["--model_name_or_path", merged, "--synthetic_data", "--synthetic_samples", "60", "--max_length", "1024",
                          "--max_prompt_length", "256", "--output_dir", str(tmp_path / "dpo"), "--max_steps", "1",
                          "--per_device_train_batch_size", "2", "--gradient_accumulation_steps", "1", "--lion",
                          "--async_grad", "--use_cpu", "--torch_dtype", "float32", "--eval_steps", "0",
                          "--warmup_steps", "1", "--logging_steps", "1", "--load_in_4bit"])
    assert tr.state.global_step == 1
    assert isinstance(tr.model.model.layers[0].mlp.down_proj, Linear4bit)


def test_linear4bit_survives_model_dtype_cast():
    m = quantize_model(_tiny(), QuantConfig())
    l4 = m.model.layers[0].self_attn.k_proj
    before = l4.dequantize(torch.float32)
    m.to(dtype=torch.bfloat16)
    assert l4.absmax.dtype == torch.float32 and l4.quant_map.dtype == torch.float32
    assert l4.qweight.dtype == torch.uint8
    assert torch.equal(l4.dequantize(torch.float32), before)


def test_quantize_after_lora_keeps_adapters_trainable():
    m = _tiny()
    inject_lora(m, LoraConfig(r=8, lora_alpha=16, lora_dropout=0.0))
    quantize_model(m, QuantConfig())
    q = m.model.layers[0].self_attn.q_proj
    assert isinstance(q.base_layer, Linear4bit)
    assert type(q.lora_A) is nn.Linear and q.lora_A.weight.requires_grad
    ids = torch.randint(0, 512, (1, 64))
    m(input_ids=ids, labels=ids).loss.backward()
    assert q.lora_B.weight.grad is not None


# ---------------------------------------------------------------------------
# The hand-built inputs of test_quant_gpu.py's edge cases (quant_edge_cases.py):
# they contain the ties and the fp16 range ends they claim, and the bit
# comparison against the oracle rejects the two planted defects.


def _quantize_last_minimum(w, code):
    """quantize_4bit_ref with the tie rule ``<=``: the LAST minimum wins."""
    blocks = w.detach().reshape(-1, 64).float()
    absmax = blocks.abs().amax(dim=1)
    safe = torch.where(absmax > 0, absmax, torch.ones_like(absmax))
    x = torch.where(absmax[:, None] > 0, blocks / safe[:, None], torch.zeros_like(blocks))
    idx = (15 - (x.unsqueeze(-1) - code).abs().flip(-1).argmin(dim=-1)).to(torch.uint8).reshape(-1, 2)
    return ((idx[:, 0] << 4) | idx[:, 1]).contiguous(), absmax


def test_tie_points_are_true_ties():
    fp4, nf4 = tie_points("fp4"), tie_points("nf4")
    h = float(code_tensor("fp4")[1]) / 2
    assert fp4 == [-h, h] and len(nf4) == 6
    for qt, pts in (("fp4", fp4), ("nf4", nf4)):
        code = code_tensor(qt)
        for t in pts:
            d = (torch.tensor(t) - code).abs()
            assert int((d == d.min()).sum()) >= 2, (qt, t)
    # 0.375 is midway between FP4's 0.25 and 0.5 in exact arithmetic, but 0.3333 (index 4) is nearer: no tie
    code = code_tensor("fp4")
    d = (torch.tensor(0.375) - code).abs()
    assert d[7] == d[5] == 0.125 and int(d.argmin()) == 4 and d[4] < 0.05
    # x = 0 under FP4: +0 (index 0) and -0 (index 8) are both at distance 0
    d0 = (torch.tensor(0.0) - code).abs()
    assert d0[0] == 0 and d0[8] == 0 and int(d0.argmin()) == 0
    # the negative half-step is a three-way tie
    dn = (torch.tensor(-h) - code).abs()
    assert dn[0] == dn[8] == dn[9] == dn.min()


@pytest.mark.parametrize("qt", ["nf4", "fp4"])
@pytest.mark.parametrize("dt", DTYPES)
def test_crafted_blocks_hold_what_they_claim(dt, qt):
    w = crafted_blocks(qt, dt)
    f = w.float()
    assert w.shape == (9, 64) and f[0].abs().max() == 1 and f[2].abs().max() == 3 and f[2].min() == -3
    assert bool((f[1] == 0).sum() == 63) and bool(torch.signbit(f[1]).any()) and bool((~torch.signbit(f[1])).any())
    assert f[3].unique().numel() == 1 and f[4].unique().numel() == 1 and bool((f[5] == 0).all())
    tiny = torch.finfo(dt).tiny
    if dt != torch.float32:
        assert bool(((f[7] != 0) & (f[7].abs() < tiny)).sum() == 63)  # subnormals of dt
    assert float(f[6].abs().max()) >= (65504.0 if dt == torch.float16 else 3.0e38)
    # defect: tie rule <= instead of <.  Differs from the oracle in the crafted tie blocks and nowhere else
    code = code_tensor(qt)
    q, a = quantize_4bit_ref(w, code)
    ql, al = _quantize_last_minimum(w, code)
    assert torch.equal(a, al)
    differ = (q != ql).view(-1, 32).any(1)
    expect = torch.zeros(9, dtype=torch.bool)
    if qt == "fp4":
        expect[[0, 1, 5, 8]] = True  # every block with an exact zero (0 ties with -0), and block 0's half steps
        expect[2] = bool((f[2] == 0).any())
        expect[7] = bool((f[7] == 0).any())
        expect[6] = bool((f[6] == 0).any())
    elif dt == torch.float32:
        expect[0] = True  # NF4's fp32-exact midpoints
    assert torch.equal(differ, expect), differ
    if bool(expect.any()):
        with pytest.raises(AssertionError, match="elements differ"):
            assert_bits(ql, q, "last minimum")
    # ... on random weights the two rules agree under NF4 (the old tests could not tell them apart); under FP4
    # they differ almost only in which zero is taken (index 0 or 8: every x nearest to 0 is a tie of +0 and -0)
    torch.manual_seed(0)
    wr = (torch.randn(384, 1024) * 0.02).to(dt)
    qa, qb = _quantize_last_minimum(wr, code)[0], quantize_4bit_ref(wr, code)[0]
    if qt == "nf4":
        assert torch.equal(qa, qb)
    else:
        ia, ib = torch.stack([qa >> 4, qa & 15], 1), torch.stack([qb >> 4, qb & 15], 1)
        diff = ia != ib
        assert bool(diff.any()) and float(((ia == 8) & (ib == 0))[diff].double().mean()) > 0.99


def _to_f16_flushing(v32):
    h = v32.to(torch.float16)
    return torch.where(h.abs() < 2.0 ** -14, torch.copysign(torch.zeros_like(h), h), h)


@pytest.mark.parametrize("qt", ["nf4", "fp4"])
def test_edge_packed_reaches_the_fp16_range_ends(qt):
    q, absmax = edge_packed()
    assert torch.equal(torch.unique(q), torch.arange(256, dtype=torch.uint8)) and absmax.unique().numel() == len(EDGE_ABSMAX)
    code = code_tensor(qt)
    v32 = dequantize_4bit_ref(q, absmax, code, torch.float32)
    h = dequantize_4bit_ref(q, absmax, code, torch.float16)
    assert torch.isfinite(v32).all() and torch.isfinite(dequantize_4bit_ref(q, absmax, code, torch.bfloat16).float()).all()
    sub = (h != 0) & (h.abs() < 2.0 ** -14)
    under = (h == 0) & (v32 != 0)
    assert bool(sub.any()) and bool((under & torch.signbit(h)).any()) and bool((under & ~torch.signbit(h)).any())
    assert bool((h == float("inf")).any()) and bool((h == float("-inf")).any())
    assert bool((h.float() != v32)[torch.isfinite(h) & ~sub & ~under].any())  # normal results that had to round
    one = code == 1.0
    for am, want in ((65504.0, 65504.0), (65519.0, 65504.0), (65520.0, float("inf")), (3.0e38, float("inf"))):
        got = (code[one] * torch.tensor(am)).to(torch.float16)
        assert float(got) == want, (am, float(got))
        assert bool(((absmax.repeat_interleave(64) == am) & (h == want)).any())
    # 0.0052 * 0.005 is already an fp16 subnormal
    if qt == "fp4":
        v = (code[1] * torch.tensor(0.005)).to(torch.float16)
        assert 0 < float(v) < 2.0 ** -14
    # defect: fp16 subnormals flushed to zero -- rejected by the bit comparison; equal on ordinary weights
    with pytest.raises(AssertionError, match="elements differ"):
        assert_bits(_to_f16_flushing(v32), h, "flushed")
    torch.manual_seed(0)
    qr, ar = quantize_4bit_ref(torch.randn(64, 1024) * 0.02, code_tensor("nf4"))
    vr = dequantize_4bit_ref(qr, ar, code_tensor("nf4"), torch.float32)
    nz = vr != 0
    assert torch.equal(_to_f16_flushing(vr)[nz], vr.to(torch.float16)[nz])


def test_dequant_sizes_leave_one_two_and_three_live_steps():
    live = [((w % 1024) + 255) // 256 for w in DEQUANT_WORDS]
    assert DEQUANT_WORDS[:3] == [64 // 8, 64 * 129 // 8, (8 * (1024 * 3 + 5) + 63) // 64 * 64 // 8]
    assert sorted(set(live)) == [1, 2, 3] and all(w % 1024 % 256 != 0 for w in DEQUANT_WORDS)
    q, a = random_packed(5, 0)
    assert q.numel() == 160 and a.numel() == 5 and bool((a > 0).all())
