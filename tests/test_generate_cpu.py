"""generate() and the KV cache on the CPU, in fp32 through the PyTorch forms: greedy generation equals the naive
loop that re-runs the full forward on the growing sequence, token for token, for every native family, for equal,
left-padded and right-padded prompts; the cached path's per-step logits match the full forward's; the stock HF
classes generate the same tokens; EOS / pad, sampling and the argument checks; and the PyTorch forms of
decode_attention / kv_append in bf16 meet the bounds and bit-checks of the GPU tests (tests/decode_cases.py)."""
import tempfile

import pytest
import torch
import transformers

import decode_cases as dc
from distributed_lion_pytorch_amd.models import KVCache, lora
from distributed_lion_pytorch_amd.models import llama as L
from distributed_lion_pytorch_amd.models.generation import warp_logits
from distributed_lion_pytorch_amd.models.gpt2 import GPT2LMHeadModel, gpt2_config
from distributed_lion_pytorch_amd.ops import fused

CPU = torch.device("cpu")


def _small(cls, **kw):
    return cls(vocab_size=97, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
               num_key_value_heads=2, max_position_embeddings=128, **kw)


def _randomise(model, names, std, seed=5):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if any(k in n for k in names):
                p.add_(std * torch.randn(p.shape, generator=g))


def _build(family, seed=0):
    torch.manual_seed(seed)
    if family == "gpt2":
        m = GPT2LMHeadModel(gpt2_config("gpt2-tiny", resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0))
    elif family == "llama":  # 2 query heads on 1 kv head
        m = L.LlamaForCausalLM(L.llama_config("llama-tiny"))
    elif family == "mistral":  # window 8 < prompt + new tokens
        m = L.MistralForCausalLM(_small(transformers.MistralConfig, sliding_window=8))
    elif family == "qwen2":  # q / k / v biases
        m = L.Qwen2ForCausalLM(_small(transformers.Qwen2Config, tie_word_embeddings=True))
        _randomise(m, ("q_proj.bias", "k_proj.bias", "v_proj.bias"), 0.1)
    elif family == "qwen3":  # q / k norm, head_dim 32 != hidden / heads
        m = L.Qwen3ForCausalLM(_small(transformers.Qwen3Config, head_dim=32, tie_word_embeddings=False))
        _randomise(m, ("q_norm", "k_norm"), 0.25)
    elif family == "llama-lora":
        m = L.LlamaForCausalLM(L.llama_config("llama-tiny"))
        lora.inject_lora(m, lora.LoraConfig(r=4, lora_alpha=8, lora_dropout=0.0))
        _randomise(m, ("lora_B",), 0.05)
    else:
        raise KeyError(family)
    return m.eval()


FAMILIES = ["gpt2", "llama", "mistral", "qwen2", "qwen3", "llama-lora"]
_MODELS = {}


def model_of(family):
    if family not in _MODELS:
        _MODELS[family] = _build(family)
    return _MODELS[family]


def _prompts(model, B, T, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, model.config.vocab_size, (B, T), generator=g)


@torch.no_grad()
def naive_greedy(model, ids, n):
    """Re-run the full forward on the growing sequence and take argmax: (ids, logits per step [n, B, V])."""
    steps = []
    for _ in range(n):
        logits = model(ids).logits[:, -1]
        steps.append(logits)
        ids = torch.cat([ids, logits.argmax(-1, keepdim=True)], dim=1)
    return ids, torch.stack(steps)


@pytest.mark.parametrize("family", FAMILIES)
def test_greedy_equals_the_naive_loop(family):
    m = model_of(family)
    ids = _prompts(m, 3, 12)
    ref, _ = naive_greedy(m, ids, 10)
    out = m.generate(ids, max_new_tokens=10)
    assert out.dtype == torch.long and torch.equal(out, ref), (out[:, 12:], ref[:, 12:])


@pytest.mark.parametrize("family", FAMILIES)
def test_ragged_prompts_left_and_right_padded(family):
    """Rows of 5, 12 and 9 tokens in a width of 12: both paddings give what each row gives alone, unpadded; the
    prompt comes back exactly as given (pad ids included)."""
    m = model_of(family)
    lens, T, n, pad = (5, 12, 9), 12, 9, 0
    rows = [_prompts(m, 1, k, seed=10 + k) for k in lens]
    alone = [naive_greedy(m, r, n)[0][0, k:] for r, k in zip(rows, lens)]
    for side in ("left", "right"):
        ids = torch.full((3, T), pad, dtype=torch.long)
        mask = torch.zeros(3, T, dtype=torch.long)
        for b, (r, k) in enumerate(zip(rows, lens)):
            sl = slice(T - k, T) if side == "left" else slice(0, k)
            ids[b, sl] = r[0]
            mask[b, sl] = 1
        out = m.generate(ids, attention_mask=mask, max_new_tokens=n)
        assert torch.equal(out[:, :T], ids), side
        for b in range(3):
            assert torch.equal(out[b, T:], alone[b]), (family, side, b, out[b, T:], alone[b])


@pytest.mark.parametrize("family", FAMILIES)
def test_cached_logits_match_the_full_forward(family):
    """Prefill + 8 decode steps on forced tokens, ragged lengths (4, 9, 7): every step's logits are the full
    forward's at that row's position, to 1e-5."""
    m = model_of(family)
    lens, steps = torch.tensor([4, 9, 7]), 8
    seq = _prompts(m, 3, 9 + steps, seed=3)
    rows = torch.arange(3)
    with torch.no_grad():
        full = m(seq).logits  # causal: the logits at position t see tokens <= t only
        cache = KVCache(m.config, 3, 9 + steps, CPU, torch.float32)
        prompt = torch.where(torch.arange(9)[None] < lens[:, None], seq[:, :9], torch.zeros_like(seq[:, :9]))
        got = m(prompt, cache=cache).logits[rows, lens - 1]
        cache.set_lengths(lens)
        worst = float((got - full[rows, lens - 1]).abs().max())
        for s in range(steps):
            pos = lens + s
            got = m(seq[rows, pos][:, None], cache=cache).logits[:, 0]
            worst = max(worst, float((got - full[rows, pos]).abs().max()))
    print(f"[generate] {family}: cached vs full logits, max abs diff {worst:.2e}")
    assert worst <= 1e-5
    assert cache.width == 9 + steps and cache.lengths.tolist() == (lens + steps).tolist()
    with pytest.raises(ValueError, match="full"), torch.no_grad():
        m(seq[:, :1], cache=cache)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_same_tokens_as_hf_generate(family):
    m = _build(family, seed=2)
    with tempfile.TemporaryDirectory() as d:
        m.save_pretrained(d)
        cls = transformers.GPT2LMHeadModel if family == "gpt2" else transformers.LlamaForCausalLM
        hf = cls.from_pretrained(d).eval()
    ids = _prompts(m, 2, 10, seed=4)
    hf.generation_config.eos_token_id = None
    with torch.no_grad():
        ref = hf.generate(ids, do_sample=False, max_new_tokens=12, min_new_tokens=12, pad_token_id=0)
    assert torch.equal(m.generate(ids, max_new_tokens=12), ref)


def _expected_with_eos(free_new, eos, pad):
    """What generate returns for the free run's new tokens once rows stop at their first EOS."""
    B, n = free_new.shape
    out = free_new.clone()
    ends = []
    for b in range(B):
        hits = [i for i in range(n) if int(free_new[b, i]) in eos]
        if hits:
            out[b, hits[0] + 1:] = pad
            ends.append(hits[0])
        else:
            ends.append(n)
    keep = max(ends) + 1 if max(ends) < n else n
    return out[:, :keep]


def test_eos_pads_finished_rows_and_ends_early(monkeypatch):
    m = model_of("llama")
    ids, T, n = _prompts(m, 3, 8, seed=6), 8, 20
    free = m.generate(ids, max_new_tokens=n)[:, T:]
    # one row stops, the others go on
    eos = int(free[0, 2])
    out = m.generate(ids, max_new_tokens=n, eos_token_id=eos, pad_token_id=7)
    exp = _expected_with_eos(free, {eos}, 7)
    assert torch.equal(out[:, T:], exp) and bool((out[0, T + 3:] == 7).all())
    assert torch.equal(m.generate(ids, max_new_tokens=n, eos_token_id=eos)[:, T:], _expected_with_eos(free, {eos}, eos))
    # every row stops by step 3: the loop leaves at the first 8-step check, the result ends where the last row did
    stop = sorted({int(free[b, 1 + b]) for b in range(3)})
    exp = _expected_with_eos(free, set(stop), 7)
    assert exp.shape[1] <= 4
    calls = []
    real = type(m.model).forward
    monkeypatch.setattr(type(m.model), "forward", lambda self, *a, **kw: (calls.append(1), real(self, *a, **kw))[1])
    out = m.generate(ids, max_new_tokens=n, eos_token_id=stop, pad_token_id=7)
    assert torch.equal(out[:, T:], exp)
    assert len(calls) == 8  # the prefill and 7 decode steps, not 20


def test_sampling():
    m = model_of("qwen2")
    ids, T, n = _prompts(m, 3, 8, seed=7), 8, 10
    greedy = m.generate(ids, max_new_tokens=n)
    assert torch.equal(m.generate(ids, max_new_tokens=n, do_sample=True, top_k=1, seed=0), greedy)
    kw = dict(max_new_tokens=n, do_sample=True, temperature=0.7, top_k=5, top_p=0.8)
    a, b, c = m.generate(ids, seed=11, **kw), m.generate(ids, seed=11, **kw), m.generate(ids, seed=12, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    # every sampled token lies in the set recomputed from the full forward's logits on its prefix
    with torch.no_grad():
        for t in range(T, T + n):
            logits = m(a[:, :t]).logits[:, -1].double() / 0.7
            top = logits.topk(5, dim=-1)
            p = top.values.softmax(-1)  # descending
            before = p.cumsum(-1) - p
            for r in range(3):
                allowed = {int(top.indices[r, j]) for j in range(5) if float(before[r, j]) < 0.8}
                assert int(a[r, t]) in allowed, (t, r, int(a[r, t]), allowed)
    # the warper alone: temperature, then top-k, then top-p
    w = warp_logits(torch.tensor([[0.0, 1.0, 2.0, 3.0]]), temperature=0.5, top_k=3, top_p=0.9)
    assert torch.isinf(w[0, 0]) and w[0, 3] == 6.0 and torch.isfinite(w[0, 2])


def test_argument_errors():
    g = model_of("gpt2")
    ids = _prompts(g, 2, 6)
    with pytest.raises(ValueError, match="contiguous"):
        g.generate(ids, attention_mask=torch.tensor([[1, 0, 1, 1, 1, 1], [1] * 6]), max_new_tokens=2)
    with pytest.raises(ValueError, match="contiguous"):
        g.generate(ids, attention_mask=torch.tensor([[0] * 6, [1] * 6]), max_new_tokens=2)
    with pytest.raises(ValueError, match="positions"):
        g.generate(ids, max_new_tokens=g.config.n_positions - 5)
    assert g.generate(ids, max_new_tokens=g.config.n_positions - 6).shape == (2, g.config.n_positions)
    g.train()
    try:
        with pytest.raises(ValueError, match="training"):
            g.generate(ids, max_new_tokens=2)
    finally:
        g.eval()
    with pytest.raises(RuntimeError, match="no_grad"):
        g(ids, cache=KVCache(g.config, 2, 8, CPU))


# ----------------------------------------------------- the PyTorch forms of the two ops, bf16 on the CPU
@pytest.mark.parametrize("D", dc.DIMS)
def test_decode_attention_torch_form_meets_the_gpu_bound(D):
    """The bound of tests/test_decode_attention_gpu.py is reachable by the reference alone."""
    for H, Hkv in dc.HEADS:
        for lens in dc.length_sets(Hkv):
            dc.check_attention_case(fused.decode_attention, CPU, D, H, Hkv, lens, splits=(None,))
    for window, lens in dc.WINDOW_CASES:
        dc.check_attention_case(fused.decode_attention, CPU, D, 8, 2, lens, window=window, splits=(None,))
    dc.check_attention_case(fused.decode_attention, CPU, D, 8, 2, (200, 250, 77), max_len=200, splits=(None,))
    dc.check_attention_case(fused.decode_attention, CPU, D, 4, 4, (200, 1, 199), window=16, max_len=200,
                            splits=(None,), shared_cache=True)


@pytest.mark.parametrize("D", dc.DIMS)
def test_kv_append_torch_form_meets_the_gpu_bit_checks(D):
    for gains in (False, True):
        dc.check_append(fused.kv_append, CPU, D, gains)
    dc.check_append(fused.kv_append, CPU, D, gains=False, tables=False)
    qkv, gq, gk, cos, sin = dc.append_inputs(D)
    q, k, v = dc.split_step(qkv, D)
    kc, kbuf = dc.guarded_cache(D, CPU)
    vc, vbuf = dc.guarded_cache(D, CPU)
    with pytest.raises(ValueError, match="KV cache"):
        fused.kv_append(q, k, v, torch.tensor([0, dc.APPEND_TMAX, 1, 2], dtype=torch.int32), cos, sin, None, None,
                        dc.APPEND_EPS, kc, vc)
    assert bool((kbuf == dc.POISON).all()) and bool((vbuf == dc.POISON).all())
