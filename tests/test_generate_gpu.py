"""Generation on the GPU in bf16 with kernel-eligible tiny models (hidden 256, 2 layers; GPT-2 at head_dim 64,
Llama at head_dim 128 with GQA 4:1, a Mistral window, Qwen3): the cached path (prefill + decode steps through
csrc/decode.hip) against the full forward, both judged on the same model in fp32 through the PyTorch forms;
generate's shape, EOS / pad semantics and repeatability; NaN beyond the rows' lengths never reaches an output.
docs/TEST_TOLERANCES.md "Generation" has the condition and the measured ratios."""
import pytest
import torch
import transformers

from distributed_lion_pytorch_amd.models import KVCache
from distributed_lion_pytorch_amd.models import llama as L
from distributed_lion_pytorch_amd.models.gpt2 import GPT2LMHeadModel, gpt2_config
from distributed_lion_pytorch_amd.ops import fused, hip

pytestmark = pytest.mark.gpu

FAMILIES = ["gpt2", "llama", "mistral", "qwen3"]
SEQ, LENS = 96, (17, 64, 65)
# the cached path's logit error may be this many times the full bf16 forward's at the same position: both are bf16
# paths of the same depth, so a larger factor is a wrong key, position or length, not rounding
MAX_RATIO = 2.0


def _llama_kw(**kw):
    return dict(vocab_size=256, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                num_key_value_heads=1, head_dim=128, max_position_embeddings=512, tie_word_embeddings=False, **kw)


def _build(family):
    torch.manual_seed(0)
    if family == "gpt2":
        m = GPT2LMHeadModel(gpt2_config("gpt2", n_embd=256, n_layer=2, n_head=4, vocab_size=256, n_positions=256,
                                        resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0, bos_token_id=0, eos_token_id=0))
    elif family == "llama":
        m = L.LlamaForCausalLM(transformers.LlamaConfig(**_llama_kw()))
    elif family == "mistral":
        m = L.MistralForCausalLM(transformers.MistralConfig(**_llama_kw(sliding_window=32)))
    else:
        m = L.Qwen3ForCausalLM(transformers.Qwen3Config(**{**_llama_kw(), "num_key_value_heads": 2}))
        g = torch.Generator().manual_seed(4)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if "q_norm" in n or "k_norm" in n:
                    p.copy_(1.0 + 0.25 * torch.randn(p.shape, generator=g))
    return m.eval()


_PAIRS = {}


def pair(family, device):
    """(the model in bf16, the same weights in fp32), built once."""
    if family not in _PAIRS:
        m = _build(family)
        ref = _build(family)
        ref.load_state_dict(m.state_dict())
        m = m.to(device, torch.bfloat16)
        ref.load_state_dict({k: v.float() for k, v in m.state_dict().items()})  # the bf16-rounded weights, in fp32
        _PAIRS[family] = (m, ref.to(device))
    return _PAIRS[family]


def _kernels_only(monkeypatch):
    monkeypatch.setattr(fused, "decode_attention_reference", lambda *a, **kw: pytest.fail("PyTorch decode_attention ran"))
    monkeypatch.setattr(fused, "kv_append_reference", lambda *a, **kw: pytest.fail("PyTorch kv_append ran"))


def _teacher_forced(m, seq, lens, poison=False):
    """Logits of the cached path at every (row, position) from lens[b] - 1 on: [B, SEQ, V] (NaN where not computed).
    poison: every cache element at and beyond a row's length is NaN before the prefill's copy and again after it."""
    B, dev = seq.shape[0], seq.device
    W, steps = max(LENS), SEQ - min(LENS)
    rows = torch.arange(B, device=dev)
    cache = KVCache(m.config, B, W + steps, dev, m.lm_head.weight.dtype)
    if poison:
        cache._buf.fill_(float("nan"))
    out = torch.full((B, SEQ, m.config.vocab_size), float("nan"), device=dev)
    with torch.no_grad():
        prompt = torch.where(torch.arange(W, device=dev)[None] < lens[:, None], seq[:, :W], torch.zeros_like(seq[:, :W]))
        out[rows, lens - 1] = m(prompt, cache=cache).logits[rows, lens - 1].float()
        cache.set_lengths(lens)
        if poison:
            for b in range(B):
                cache._buf[:, :, b, int(lens[b]):] = float("nan")
        for s in range(steps):
            pos = lens + s
            live = pos < SEQ
            tok = seq[rows, pos.clamp_max(SEQ - 1)]
            logits = m(tok[:, None], cache=cache).logits[:, 0].float()
            out[rows[live], pos[live]] = logits[live]
    return out


@pytest.mark.parametrize("family", FAMILIES)
def test_teacher_forced_consistency(family, cuda, monkeypatch):
    hip.require()
    m, ref = pair(family, cuda)
    seq = torch.randint(1, 256, (3, SEQ), generator=torch.Generator().manual_seed(9)).to(cuda)
    lens = torch.tensor(LENS, device=cuda)
    fused.set_impl("torch")
    try:
        with torch.no_grad():
            exact = ref(seq).logits.float()
    finally:
        fused.set_impl("auto")
    with torch.no_grad():
        full = m(seq).logits.float()
    _kernels_only(monkeypatch)
    cached = _teacher_forced(m, seq, lens)
    done = ~torch.isnan(cached).any(-1)
    assert bool((done == (torch.arange(SEQ, device=cuda)[None] >= (lens - 1)[:, None])).all())
    assert bool(torch.isfinite(cached[done]).all())
    e_full = (full - exact).abs().amax(-1)
    e_cached = torch.where(done, (torch.nan_to_num(cached) - exact).abs().amax(-1), torch.zeros_like(e_full))
    ratio = torch.where(done, e_cached / e_full, torch.zeros_like(e_full))
    worst = float(ratio.max())
    b, t = (int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape))
    print(f"[generate] {family}: cached / full logit error against fp32, max ratio {worst:.3f} at row {b} position {t} "
          f"(cached {float(e_cached[b, t]):.3e}, full {float(e_full[b, t]):.3e}); median {float(ratio[done].median()):.3f}")
    assert worst <= MAX_RATIO
    fused.check_index_errors(blocking=True)


@pytest.mark.parametrize("family", ["gpt2", "qwen3"])
def test_nan_beyond_the_lengths_never_reaches_the_logits(family, cuda, monkeypatch):
    hip.require()
    _kernels_only(monkeypatch)
    m, _ = pair(family, cuda)
    seq = torch.randint(1, 256, (3, SEQ), generator=torch.Generator().manual_seed(10)).to(cuda)
    lens = torch.tensor(LENS, device=cuda)
    clean, poisoned = _teacher_forced(m, seq, lens), _teacher_forced(m, seq, lens, poison=True)
    done = ~torch.isnan(clean).any(-1)
    assert bool(torch.isfinite(poisoned[done]).all())
    assert torch.equal(clean[done], poisoned[done])


@pytest.mark.parametrize("family", FAMILIES)
def test_generate(family, cuda, monkeypatch):
    hip.require()
    _kernels_only(monkeypatch)
    m, _ = pair(family, cuda)
    T, n = 20, 24
    ids = torch.randint(1, 256, (3, T), generator=torch.Generator().manual_seed(11)).to(cuda)
    mask = torch.ones_like(ids)
    mask[0, :7] = 0  # left-padded row
    free = m.generate(ids, attention_mask=mask, max_new_tokens=n)
    assert free.shape == (3, T + n) and free.dtype == torch.long and torch.equal(free[:, :T], ids)
    assert int(free.min()) >= 0 and int(free.max()) < 256
    assert torch.equal(m.generate(ids, attention_mask=mask, max_new_tokens=n), free)
    # row 1 stops at its third new token and is padded from then on; the others continue as before until they
    # emit that token themselves
    eos = int(free[1, T + 2])
    out = m.generate(ids, attention_mask=mask, max_new_tokens=n, eos_token_id=eos, pad_token_id=255)
    new, exp = out[:, T:], free[:, T:].clone()
    ends = []
    for b in range(3):
        hits = (exp[b] == eos).nonzero()
        ends.append(int(hits[0]) if len(hits) else n)
        exp[b, ends[-1] + 1:] = 255
    keep = max(ends) + 1 if max(ends) < n else n
    assert ends[1] <= 2 and torch.equal(new, exp[:, :keep])
    a = m.generate(ids, attention_mask=mask, max_new_tokens=n, do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=5)
    b = m.generate(ids, attention_mask=mask, max_new_tokens=n, do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=5)
    assert a.shape == (3, T + n) and torch.equal(a, b)
    fused.check_index_errors(blocking=True)
