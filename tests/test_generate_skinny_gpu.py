"""Generation through the skinny-M GEMM: every weight GEMM of a decode step (projections, MLP, greedy LM head) runs
csrc/skinny_gemm.hip and none of a gradient-enabled forward does; a 4-bit base decodes straight from its 4-bit store
and meets the bf16 models' teacher-forced condition (tests/test_generate_gpu.py, whose builders are reused)."""
import copy

import pytest
import torch

import test_generate_gpu as tg

from distributed_lion_pytorch_amd.models import KVCache
from distributed_lion_pytorch_amd.models import quant as mq
from distributed_lion_pytorch_amd.ops import fused, hip

pytestmark = pytest.mark.gpu


def _count(monkeypatch, name):
    calls = []
    orig = getattr(fused, name)

    def counted(x, *a, **kw):
        calls.append((x.shape[0], x.shape[1]))
        return orig(x, *a, **kw)

    monkeypatch.setattr(fused, name, counted)
    return calls


@pytest.mark.parametrize("family", tg.FAMILIES)
def test_every_gemm_of_a_decode_step_is_the_skinny_kernel(family, cuda, monkeypatch):
    hip.require()
    m, _ = tg.pair(family, cuda)
    calls = _count(monkeypatch, "skinny_gemm")
    B, T = 3, 20
    ids = torch.randint(1, 256, (B, T), generator=torch.Generator().manual_seed(12)).to(cuda)
    base = m._decoder()
    layers = m.config.n_layer if family == "gpt2" else m.config.num_hidden_layers
    hidden = 256
    with torch.no_grad():
        cache = KVCache(m.config, B, T + 4, cuda, torch.bfloat16)
        h = base(ids, cache=cache)[:, -1]
        assert not calls, "the prefill (60 rows) is not a decode step"
        cache.set_lengths(torch.full((B,), T, device=cuda))
        ignore = torch.full((B,), -100, dtype=torch.long, device=cuda)
        tok = fused.lm_head_score(h, m.lm_head.weight, ignore).pred.long()
        assert calls == [(B, hidden)], "the greedy LM head"
        del calls[:]
        base(tok[:, None], cache=cache)
    # per layer: the fused q|k|v projection, the output projection, the MLP's two GEMMs -- but GPT-2's c_fc, which
    # keeps hipBLASLt's fused bias + GELU epilogue (one launch; the skinny kernel plus a GELU kernel would be two)
    if family == "gpt2":
        per_layer = [(B, hidden), (B, hidden), (B, 1024)]
    else:
        per_layer = [(B, hidden), (B, 512), (B, hidden), (B, 512)]
    assert calls == per_layer * layers, calls
    del calls[:]
    # sampling takes the logits from the same kernel
    with torch.no_grad():
        m.generate(ids, max_new_tokens=2, do_sample=True, top_k=5, seed=1)
    assert len(calls) == 2 + len(per_layer) * layers and calls[0] == calls[-1] == (B, hidden), calls  # two draws, one step
    del calls[:]
    # the gradient-enabled twin: a plain forward of 16 rows stays on the training path (its GEMMs run inside
    # autograd Functions, where the grad mode reads "off")
    assert torch.is_grad_enabled()
    m(ids[:2, :8])
    assert not calls, "a gradient-enabled forward took the inference kernel"
    fused.check_index_errors(blocking=True)


_Q4 = {}


def _pair4(device):
    """(the tiny Llama with an nf4 base, bf16; the same dequantised weights in an fp32 model)."""
    if not _Q4:
        m = tg._build("llama").to(device, torch.bfloat16)
        mq.quantize_model(m, bnb_4bit_quant_type="nf4")
        ref = tg._build("llama")
        sd = mq.dequantize_model(copy.deepcopy(m)).state_dict()
        ref.load_state_dict({k: v.float() for k, v in sd.items()})
        _Q4["pair"] = (m.eval(), ref.to(device).eval())
    return _Q4["pair"]


def test_4bit_teacher_forced_consistency(cuda, monkeypatch):
    hip.require()
    m, ref = _pair4(cuda)
    assert any(isinstance(x, mq.Linear4bit) for x in m.modules()) and not any(isinstance(x, mq.Linear4bit) for x in ref.modules())
    seq = torch.randint(1, 256, (3, tg.SEQ), generator=torch.Generator().manual_seed(9)).to(cuda)
    lens = torch.tensor(tg.LENS, device=cuda)
    fused.set_impl("torch")
    try:
        with torch.no_grad():
            exact = ref(seq).logits.float()
    finally:
        fused.set_impl("auto")
    with torch.no_grad():
        full = m(seq).logits.float()  # the full 4-bit bf16 forward: 288 rows, the expansion path
    tg._kernels_only(monkeypatch)
    w4 = _count(monkeypatch, "skinny_gemm_w4")
    expansions = []
    orig = mq.dequantize_4bit
    monkeypatch.setattr(mq, "dequantize_4bit", lambda *a, **kw: expansions.append(1) or orig(*a, **kw))
    cached = tg._teacher_forced(m, seq, lens)
    steps = tg.SEQ - min(tg.LENS)
    # per decode step and layer: q, k, v, o, gate, up, down, each straight from the 4-bit store; the only
    # expansions are the prefill's (q|k|v, o, gate|up, down per layer: 7 weights)
    assert len(w4) == steps * 2 * 7 and set(r for r, _ in w4) == {3}
    assert len(expansions) == 2 * 7
    done = ~torch.isnan(cached).any(-1)
    assert bool((done == (torch.arange(tg.SEQ, device=cuda)[None] >= (lens - 1)[:, None])).all())
    assert bool(torch.isfinite(cached[done]).all())
    e_full = (full - exact).abs().amax(-1)
    e_cached = torch.where(done, (torch.nan_to_num(cached) - exact).abs().amax(-1), torch.zeros_like(e_full))
    ratio = torch.where(done, e_cached / e_full, torch.zeros_like(e_full))
    worst = float(ratio.max())
    b, t = (int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape))
    print(f"[generate] llama nf4: cached / full logit error against fp32, max ratio {worst:.3f} at row {b} position {t} "
          f"(cached {float(e_cached[b, t]):.3e}, full {float(e_full[b, t]):.3e}); median {float(ratio[done].median()):.3f}")
    assert worst <= tg.MAX_RATIO
    fused.check_index_errors(blocking=True)


def test_4bit_generate_is_repeatable(cuda, monkeypatch):
    hip.require()
    tg._kernels_only(monkeypatch)
    m, _ = _pair4(cuda)
    w4 = _count(monkeypatch, "skinny_gemm_w4")
    ids = torch.randint(1, 256, (3, 20), generator=torch.Generator().manual_seed(11)).to(cuda)
    mask = torch.ones_like(ids)
    mask[0, :7] = 0
    a = m.generate(ids, attention_mask=mask, max_new_tokens=12)
    assert a.shape == (3, 32) and torch.equal(a[:, :20], ids) and len(w4) == 11 * 2 * 7
    assert torch.equal(m.generate(ids, attention_mask=mask, max_new_tokens=12), a)
    s1 = m.generate(ids, attention_mask=mask, max_new_tokens=12, do_sample=True, temperature=0.8, top_k=20, seed=5)
    s2 = m.generate(ids, attention_mask=mask, max_new_tokens=12, do_sample=True, temperature=0.8, top_k=20, seed=5)
    assert torch.equal(s1, s2)
    fused.check_index_errors(blocking=True)
