"""4-bit quantization kernels (csrc/quant.hip) against the PyTorch oracle of
ops/quant.py (identical indices / absmax, bit-identical expansion), and the
Linear4bit / QLoRA path on the GPU against fp32 PyTorch references."""
import pytest
import torch
import torch.nn as nn

from distributed_lion_pytorch_amd.models.llama import LlamaForCausalLM, llama_config
from distributed_lion_pytorch_amd.models.lora import LoraConfig, inject_lora
from distributed_lion_pytorch_amd.models.quant import Linear4bit, QuantConfig, dequantize_model, quantize_model
from distributed_lion_pytorch_amd.ops import hip
from distributed_lion_pytorch_amd.ops.quant import (code_tensor, dequantize_4bit, dequantize_4bit_ref, quantize_4bit,
                                                    quantize_4bit_ref)
from numerics import assert_bits
from quant_edge_cases import (DEQUANT_T_SHAPES, DEQUANT_WORDS, DTYPES, EDGE_ABSMAX, QUANT_BLOCKS, crafted_blocks,
                              edge_packed, random_packed, tie_points)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("qt", ["nf4", "fp4"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
def test_quant4_kernel_matches_oracle(cuda, qt, dt):
    hip.require()
    torch.manual_seed(0)
    w = (torch.randn(384, 1024, device=cuda) * 0.02).to(dt)
    w[3, :64] = 0  # an all-zero block
    code = code_tensor(qt, cuda)
    q, a = quantize_4bit(w, code)
    qr, ar = quantize_4bit_ref(w, code)
    assert torch.equal(a, ar)
    assert torch.equal(q, qr)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
def test_dequant4_kernel_bit_exact(cuda, dt):
    hip.require()
    torch.manual_seed(0)
    # 20000 x 4096: 2.56M work items > one grid (exercises the grid-stride loop)
    w = torch.randn(20000, 4096, device=cuda, dtype=torch.bfloat16)
    code = code_tensor("nf4", cuda)
    q, a = quantize_4bit(w, code)
    d = dequantize_4bit(q, a, code, w.shape, dt)
    assert torch.equal(d.view(-1), dequantize_4bit_ref(q, a, code, dt))
    # into a row block of a bigger buffer (the fused projection layout)
    big = torch.full((20000 + 128, 4096), 7.0, device=cuda, dtype=dt)
    dequantize_4bit(q, a, code, w.shape, dt, out=big[64:64 + 20000])
    assert torch.equal(big[64:64 + 20000], d)
    assert (big[:64] == 7).all() and (big[-64:] == 7).all()


def test_linear4bit_fwd_bwd_vs_fp32(cuda):
    hip.require()
    torch.manual_seed(0)
    lin = nn.Linear(1024, 768, bias=False, device=cuda, dtype=torch.bfloat16)
    q4 = Linear4bit.from_linear(lin)
    wref = q4.dequantize(torch.float32)
    x = torch.randn(4, 256, 1024, device=cuda, dtype=torch.bfloat16, requires_grad=True)
    y = q4(x)
    g = torch.randn_like(y)
    y.backward(g)
    xr = x.detach().float().requires_grad_()
    yr = xr @ wref.t()
    yr.backward(g.float())
    assert (y.float() - yr).abs().max().item() < 2e-2 * yr.abs().max().item()
    assert (x.grad.float() - xr.grad).abs().max().item() < 2e-2 * xr.grad.abs().max().item()


def test_qlora_llama_gpu_matches_dequantized(cuda):
    """QLoRA step on the GPU (fused q/k/v + gate/up 4-bit GEMMs, LoRA kernels)
    equals LoRA over the dequantized bf16 weights."""
    hip.require()
    cfg = llama_config("llama-tiny", hidden_size=256, intermediate_size=768, num_attention_heads=4,
                       num_key_value_heads=2)

    def make():
        torch.manual_seed(0)
        with torch.device(cuda):
            return LlamaForCausalLM(cfg).to(torch.bfloat16)

    m4 = quantize_model(make(), QuantConfig(bnb_4bit_compute_dtype=torch.bfloat16))
    mr = dequantize_model(quantize_model(make(), QuantConfig(bnb_4bit_compute_dtype=torch.bfloat16)))
    lc = LoraConfig(r=8, lora_alpha=16, lora_dropout=0.0, target_modules=["q_proj", "v_proj"])
    torch.manual_seed(1)
    inject_lora(m4, lc)
    torch.manual_seed(1)
    inject_lora(mr, lc)
    byname = dict(mr.named_parameters())
    with torch.no_grad():
        for n, p in m4.named_parameters():
            if "lora_" in n:
                if "lora_B" in n:
                    p.normal_(0, 0.02)
                byname[n].copy_(p)
    ids = torch.randint(0, cfg.vocab_size, (2, 128), device=cuda)
    l4 = m4(input_ids=ids, labels=ids).loss
    lr = mr(input_ids=ids, labels=ids).loss
    assert abs(l4.item() - lr.item()) < 1e-2
    l4.backward()
    lr.backward()
    for n, p in m4.named_parameters():
        if p.requires_grad:
            gr = byname[n].grad.float()
            assert (p.grad.float() - gr).abs().max().item() <= 5e-2 * gr.abs().max().item() + 1e-6, n


def test_dequant4_transposed_into_column_blocks(cuda):
    """The transposed expansion (input-gradient GEMM layout) equals the plain
    one transposed, written into a column block of a concatenated W^T."""
    hip.require()
    torch.manual_seed(1)
    code = code_tensor("nf4", cuda)
    w = torch.randn(1024, 768, device=cuda, dtype=torch.bfloat16)
    q, a = quantize_4bit(w, code)
    full = dequantize_4bit(q, a, code, w.shape, torch.bfloat16)
    big = torch.full((768, 3 * 1024), 5.0, device=cuda, dtype=torch.bfloat16)
    hip.ops().dequant4_t_(q, a, code, big[:, 1024:2048])
    assert torch.equal(big[:, 1024:2048], full.t())
    assert (big[:, :1024] == 5).all() and (big[:, 2048:] == 5).all()


# ---------------------------------------------------------------------------
# Edges of csrc/quant.hip (docs/TEST_TOLERANCES.md "LoRA and 4-bit"): sizes
# that make the tail guards fire, crafted blocks for the tie rule and the sign
# of zero, and hand-built packed inputs that drive the fp16 expansion to
# subnormals, underflow and overflow.  Everything is bit-exact against the
# PyTorch oracle, evaluated on the GPU and on a CPU copy of the inputs, so the
# expectation does not depend on the GPU's PyTorch.


def _check_quant4(w, qt, name):
    """quant4 on the GPU copy of ``w`` (CPU) == the oracle on the GPU == the oracle on the CPU."""
    hip.require()
    dev = torch.device("cuda", 0)
    wg = w.to(dev)
    q, a = hip.ops().quant4(wg, code_tensor(qt, dev))
    assert q.dtype == torch.uint8 and q.shape == (w.numel() // 2,) and a.shape == (w.numel() // 64,)
    for where, (qr, ar) in (("gpu oracle", quantize_4bit_ref(wg, code_tensor(qt, dev))),
                            ("cpu oracle", quantize_4bit_ref(w, code_tensor(qt)))):
        assert_bits(a.cpu(), ar.cpu(), f"{name} absmax vs {where}")
        bad = (q.cpu() != qr.cpu()).nonzero().flatten().tolist()
        assert not bad, (f"{name}: {len(bad)} bytes differ from the {where}; first: byte {bad[0]} (block {bad[0] // 32}) "
                         f"got {int(q[bad[0]]):#04x} expected {int(qr[bad[0]]):#04x}")
    return q, a


@pytest.mark.parametrize("qt", ["nf4", "fp4"])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nblocks", QUANT_BLOCKS)
def test_quant4_block_counts(cuda, nblocks, dt, qt):
    """1, 255, 256, 257 blocks: the b >= nblocks guard with 255, 1, 0 and 255 idle threads."""
    g = torch.Generator().manual_seed(nblocks)
    w = (torch.randn(nblocks, 64, generator=g) * 0.02).to(dt)
    _check_quant4(w, qt, f"quant4 {nblocks} blocks {dt} {qt}")


@pytest.mark.parametrize("qt", ["nf4", "fp4"])
@pytest.mark.parametrize("dt", DTYPES)
def test_quant4_crafted_blocks(cuda, dt, qt):
    """Blocks of absmax 1 holding the exact midpoints between two nearest codes (first minimum wins; six of NF4's
    adjacent pairs have an fp32-exact midpoint, FP4 has +-code[1] / 2 -- the negative one a three-way tie with +0
    and -0 -- and x = 0 itself, equidistant from index 0 and index 8), +-0.0 inputs, a negative maximum, a repeated
    value, an all-zero block next to the largest finite values, subnormal inputs.  0.375 is midway between FP4's
    0.25 and 0.5 but nearest to 0.3333 (index 4): no tie, it is in the block all the same.  NaN and inf inputs are
    out of scope: the oracle's argmin over NaN distances is not a contract the kernel follows."""
    w = crafted_blocks(qt, dt)
    q, a = _check_quant4(w, qt, f"quant4 crafted {dt} {qt}")
    idx = torch.stack([q.cpu() >> 4, q.cpu() & 15], 1).reshape(-1, 64)
    if qt == "fp4":
        zero = (w[1].float() == 0).nonzero().flatten()
        assert zero.numel() == 63 and bool((idx[1][zero] == 0).all())  # +0 and -0 both go to index 0, never to 8
        assert bool((idx[0][w[0].float() == 0.375] == 4).all())
        if dt == torch.float32:
            half = w[0].abs() == tie_points("fp4")[1]
            assert int(half.sum()) >= 2 and bool((idx[0][half] == 0).all())  # not 1, 8 or 9
    elif dt == torch.float32:
        code = code_tensor("nf4")
        for t in tie_points("nf4"):
            lo = int((code < t).sum()) - 1  # the lower neighbour has the smaller index in NF4's ascending table
            hit = w[0] == t
            assert int(hit.sum()) >= 1 and bool((idx[0][hit] == lo).all()), t
    assert a[5] == 0 and bool((q.cpu().view(-1, 32)[5] == (0x77 if qt == "nf4" else 0x00)).all())


def _check_dequant4(q, absmax, qt, dt, name):
    hip.require()
    dev = torch.device("cuda", 0)
    out = torch.empty(2 * q.numel(), dtype=dt, device=dev)
    hip.ops().dequant4_(q.to(dev), absmax.to(dev), code_tensor(qt, dev), out)
    assert_bits(out.cpu(), dequantize_4bit_ref(q.to(dev), absmax.to(dev), code_tensor(qt, dev), dt).cpu(), f"{name} vs gpu oracle")
    exp = dequantize_4bit_ref(q, absmax, code_tensor(qt), dt)
    assert_bits(out.cpu(), exp, f"{name} vs cpu oracle")
    return exp


@pytest.mark.parametrize("qt", ["nf4", "fp4"])
@pytest.mark.parametrize("dt", DTYPES)
def test_dequant4_every_byte_every_scale(cuda, dt, qt):
    """Every byte value under absmax = 2^-30 .. 2^17, 0.005, 65504, 65519, 65520, 3e38: in fp16 the products round,
    fall into the subnormals, underflow to +-0 (sign kept) and overflow to +-inf exactly as PyTorch's conversion."""
    q, absmax = edge_packed()
    exp = _check_dequant4(q, absmax, qt, dt, f"dequant4 edges {dt} {qt}")
    if dt == torch.float16:
        assert bool(torch.isinf(exp).any()) and bool(((exp != 0) & (exp.abs() < 2.0 ** -14)).any())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("words", DEQUANT_WORDS)
def test_dequant4_tail_sizes(cuda, words, dt):
    """Word counts that are no multiple of 1024: the i < words guards fire with 1, 2 and 3 live steps."""
    assert words % 8 == 0 and words % 1024 != 0
    q, absmax = random_packed(words // 8, words)
    _check_dequant4(q, absmax, "nf4", dt, f"dequant4 {words} words {dt}")


@pytest.mark.parametrize("qt", ["nf4", "fp4"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,K", DEQUANT_T_SHAPES)
def test_dequant4_transposed_edges(cuda, N, K, dt, qt):
    """The transposed expansion into a column block between sentinel columns == the oracle's [N, K] transposed,
    on hand-built bytes and absmax values (every byte value, the fp16 range ends)."""
    hip.require()
    nb = N * K // 64
    i = torch.arange(nb * 32)
    q = ((i * 37 + i // 256) % 256).to(torch.uint8)  # every byte value, shifting against the blocks
    absmax = torch.tensor(EDGE_ABSMAX, dtype=torch.float32)[torch.arange(nb) % len(EDGE_ABSMAX)]
    assert nb >= len(EDGE_ABSMAX) and torch.unique(q).numel() == 256
    exp = dequantize_4bit_ref(q, absmax, code_tensor(qt), dt).view(N, K).t()
    big = torch.full((K, N + 24), 5.0, device=cuda, dtype=dt)
    hip.ops().dequant4_t_(q.to(cuda), absmax.to(cuda), code_tensor(qt, cuda), big[:, 8:8 + N])
    assert_bits(big[:, 8:8 + N].cpu().contiguous(), exp.contiguous(), f"dequant4_t {N}x{K} {dt} {qt}")
    assert bool((big[:, :8] == 5).all()) and bool((big[:, 8 + N:] == 5).all())


def test_dequant4_transposed_refuses_bad_shapes(cuda):
    """N % 64 != 0, K % 128 != 0 and an fp32 out raise before anything is launched."""
    hip.require()
    code = code_tensor("nf4", cuda)
    for N, K, dt in [(32, 128, torch.bfloat16), (64, 64, torch.bfloat16), (96, 256, torch.float16),
                     (64, 128, torch.float32)]:
        q = torch.zeros(N * K // 2, dtype=torch.uint8, device=cuda)
        absmax = torch.ones(N * K // 64, device=cuda)
        out = torch.full((K, N), 3.0, device=cuda, dtype=dt)
        with pytest.raises(RuntimeError, match="dlion|dequant4_t"):
            hip.ops().dequant4_t_(q, absmax, code, out)
        assert bool((out == 3).all())
