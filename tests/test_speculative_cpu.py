"""Speculative decoding and the multi-token cached forward on the CPU, in fp32 through the PyTorch forms: a chunk
forward equals single-token steps on the same cache contents; generate(assistant_model=...) is token for token
plain greedy decoding for three assistants, with and without EOS; KVCache.truncate and the ragged n_new
bookkeeping; and the PyTorch forms of chunk_attention / kv_append_chunk in bf16 meet the bounds and bit-checks of
the GPU tests (tests/chunk_cases.py)."""
import pytest
import torch
import transformers

import chunk_cases as cc
from distributed_lion_pytorch_amd.models import KVCache
from distributed_lion_pytorch_amd.models import llama as L
from distributed_lion_pytorch_amd.models.generation import SpeculativeOutput
from distributed_lion_pytorch_amd.models.gpt2 import GPT2LMHeadModel, gpt2_config
from distributed_lion_pytorch_amd.ops import fused

CPU = torch.device("cpu")
FAMILIES = ["gpt2", "llama", "mistral", "qwen3"]
MIN_MARGIN = 1e-3  # top-1 / top-2 logit margin the compared tokens must have: fp32 rounding is ~1e-6 of the logits


def _build(family, seed=0, layers=2):
    torch.manual_seed(seed)
    kw = dict(vocab_size=97, hidden_size=64, intermediate_size=128, num_hidden_layers=layers, num_attention_heads=4,
              num_key_value_heads=2, max_position_embeddings=128)
    if family == "gpt2":
        m = GPT2LMHeadModel(gpt2_config("gpt2-tiny", n_layer=layers, vocab_size=97, n_positions=64, resid_pdrop=0.0,
                                        embd_pdrop=0.0, attn_pdrop=0.0, bos_token_id=0, eos_token_id=0))
    elif family == "llama":
        m = L.LlamaForCausalLM(transformers.LlamaConfig(**kw))
    elif family == "mistral":  # window 8 < prompt + new tokens
        m = L.MistralForCausalLM(transformers.MistralConfig(sliding_window=8, **kw))
    else:
        m = L.Qwen3ForCausalLM(transformers.Qwen3Config(head_dim=32, tie_word_embeddings=False, **kw))
        g = torch.Generator().manual_seed(4 + seed)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if "q_norm" in n or "k_norm" in n:
                    p.copy_(1.0 + 0.25 * torch.randn(p.shape, generator=g))
    with torch.no_grad():  # the default init gives near-uniform logits: widen the margins
        m.lm_head.weight.mul_(8.0)
    return m.eval()


_MODELS = {}


def model_of(family, seed=0, layers=2):
    key = (family, seed, layers)
    if key not in _MODELS:
        _MODELS[key] = _build(family, seed, layers)
    return _MODELS[key]


def assistants(family):
    return {"self": model_of(family), "one layer": model_of(family, 1, 1), "other seed": model_of(family, 2)}


def _prompts(B, T, seed=1):
    return torch.randint(1, 97, (B, T), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("family", FAMILIES)
def test_chunk_forward_equals_single_steps(family):
    m = model_of(family)
    base = m._decoder()
    B, W, T = 3, 12, 5
    lens = torch.tensor((5, 12, 9))
    seq = _prompts(B, W + 2 * T, seed=3)
    prompt = torch.where(torch.arange(W)[None] < lens[:, None], seq[:, :W], torch.zeros_like(seq[:, :W]))
    with torch.no_grad():
        caches = []
        for _ in range(2):
            c = KVCache(m.config, B, W + 2 * T + 1, CPU, torch.float32)
            base(prompt, cache=c)
            c.set_lengths(lens)
            caches.append(c)
        one, chunked = caches
        feed = seq[:, W:]
        steps = torch.stack([base(feed[:, t:t + 1], cache=one)[:, 0] for t in range(T)], dim=1)
        chunk = base(feed[:, :T], cache=chunked)
        assert torch.allclose(chunk, steps, rtol=1e-5, atol=1e-5), float((chunk - steps).abs().max())
        assert torch.equal(one.lengths, chunked.lengths) and one.width == chunked.width == W + T
        # a ragged second chunk: row b keeps n[b] tokens; the other cache takes them as masked single steps
        n = torch.tensor((0, 2, T), dtype=torch.int32)
        ragged = base(feed[:, T:], cache=chunked, n_new=n)
        assert torch.equal(chunked.lengths, (lens + T + n).to(torch.int32)) and chunked.width == W + 2 * T
        for t in range(T):
            live = t < n
            before = one.lengths.clone()
            h = base(feed[:, T + t:T + t + 1], cache=one)[:, 0]
            one.truncate(torch.where(live, before + 1, before), one.width)
            assert torch.allclose(ragged[live, t], h[live], rtol=1e-5, atol=1e-5)
        assert torch.equal(one.lengths, chunked.lengths)
        kc, vc = chunked.layer(0)
        ko, vo = one.layer(0)
        for b in range(B):
            end = int(chunked.lengths[b])
            assert torch.allclose(kc[b, :end], ko[b, :end], rtol=1e-5, atol=1e-5)
            assert torch.allclose(vc[b, :end], vo[b, :end], rtol=1e-5, atol=1e-5)


def _margins(m, out, T0):
    """Top-1 / top-2 margin of the full forward at the positions that produced the new tokens: [B, n]."""
    with torch.no_grad():
        logits = m(out).logits[:, T0 - 1:-1]
    top = logits.topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]


@pytest.mark.parametrize("family", FAMILIES)
def test_speculative_equals_plain_greedy(family):
    m = model_of(family)
    T0, n = 10, 14
    ids = _prompts(3, T0, seed=2)
    plain = m.generate(ids, max_new_tokens=n)
    margin = _margins(m, plain, T0)
    assert float(margin.min()) >= MIN_MARGIN, f"{family}: choose another seed, the smallest margin is {float(margin.min()):.2e}"
    eos = int(plain[1, T0 + 2])
    plain_eos = m.generate(ids, max_new_tokens=n, eos_token_id=eos, pad_token_id=96)
    for name, a in assistants(family).items():
        for k in (1, 3, 7):
            out = m.generate(ids, max_new_tokens=n, assistant_model=a, num_assistant_tokens=k, return_dict_in_generate=True)
            assert isinstance(out, SpeculativeOutput) and out.sequences_scores is None
            assert torch.equal(out.sequences, plain), (family, name, k, out.sequences[:, T0:], plain[:, T0:])
            assert out.rounds >= 1 and out.accepted.shape == (3,)
            assert int(out.accepted.min()) >= 0 and int(out.accepted.max()) <= n - 1
            if name == "self":  # every draft is the target's own choice: ceil((n - 1) / (k + 1)) rounds
                full, rest = divmod(n - 1, k + 1)  # the first token comes from the prefill; a full round emits k + 1
                assert out.rounds == full + (rest > 0), (family, k, out.rounds)
                assert out.accepted.tolist() == [full * k + rest] * 3, (family, k, out.accepted)
        got = m.generate(ids, max_new_tokens=n, assistant_model=a, eos_token_id=eos, pad_token_id=96)
        assert torch.equal(got, plain_eos), (family, name, got[:, T0:], plain_eos[:, T0:])
    assert plain_eos.shape[1] <= T0 + n


def test_left_padded_prompts_and_the_position_limit():
    """GPT-2 with n_positions = 64: a request that fills the learned positions exactly is accepted (the last rounds
    draft fewer tokens), with a left-padded row."""
    m = model_of("gpt2")
    a = model_of("gpt2", 1, 1)
    T0, n = 40, 24
    ids = _prompts(2, T0, seed=6)
    mask = torch.ones_like(ids)
    mask[0, :9] = 0
    plain = m.generate(ids, attention_mask=mask, max_new_tokens=n)
    for assistant in (m, a):
        assert torch.equal(m.generate(ids, attention_mask=mask, max_new_tokens=n, assistant_model=assistant,
                                      num_assistant_tokens=5), plain)
    with pytest.raises(ValueError, match="learned positions"):
        m.generate(ids, max_new_tokens=n + 1, assistant_model=a)


def test_argument_checks():
    m, ids = model_of("llama"), _prompts(2, 6)
    a = model_of("llama", 1, 1)
    with pytest.raises(ValueError, match="do_sample=False"):
        m.generate(ids, max_new_tokens=4, assistant_model=a, do_sample=True)
    with pytest.raises(ValueError, match="num_beams=1"):
        m.generate(ids, max_new_tokens=4, assistant_model=a, num_beams=2)
    for k in (0, 8):
        with pytest.raises(ValueError, match="num_assistant_tokens"):
            m.generate(ids, max_new_tokens=4, assistant_model=a, num_assistant_tokens=k)
    other = L.LlamaForCausalLM(transformers.LlamaConfig(vocab_size=98, hidden_size=64, intermediate_size=128,
                                                        num_hidden_layers=1, num_attention_heads=4,
                                                        num_key_value_heads=2)).eval()
    with pytest.raises(ValueError, match="vocabulary"):
        m.generate(ids, max_new_tokens=4, assistant_model=other)
    assert m.generate(ids, max_new_tokens=1, assistant_model=a).shape == (2, 7)


_CLI = ["--model_name_or_path", "gpt2-tiny", "--prompt", "ab", "--prompt", "abcd", "--max_new_tokens", "9", "--device", "cpu"]


def test_generate_py_assistant_flags(capsys):
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import generate

    plain = generate.main(_CLI)
    assert "speculative" not in capsys.readouterr().out
    out = generate.main(_CLI + ["--assistant_model", "gpt2-tiny", "--num_assistant_tokens", "3"])
    assert out.shape[0] == plain.shape[0] == 2 and out.shape[1] <= 4 + 9
    lines =[ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[generate] speculative: ")]
    assert len(lines) == 1 and " rounds of up to 3 drafts, accepted per prompt [" in lines[0], lines


@pytest.mark.parametrize("extra", [[], ["--assistant_model", "gpt2-tiny", "--num_assistant_tokens", "4"]],
                         ids=["plain", "assistant"])
def test_generate_py_runs_as_a_script(extra):
    """The entrypoint itself, as the README calls it: exit status 0, and the summary line with an assistant."""
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, str(root / "generate.py")] + _CLI + extra, capture_output=True, text=True, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "tokens/s on cpu" in r.stdout
    assert ("[generate] speculative: " in r.stdout) == bool(extra), r.stdout


def test_cache_bookkeeping():
    m = model_of("llama")
    B, W = 2, 6
    cache = KVCache(m.config, B, 16, CPU, torch.float32)
    ids = _prompts(B, W)
    with torch.no_grad():
        with pytest.raises(ValueError, match="prefill"):
            cache.begin(B, W, torch.tensor((1, 2)))
        m._decoder()(ids, cache=cache)
        assert cache.width == W and cache.lengths.tolist() == [W, W]
        with pytest.raises(ValueError, match="1 to 8"):
            cache.begin(B, 9)
        m._decoder()(_prompts(B, 4, 2), cache=cache, n_new=torch.tensor((1, 4)))
        assert cache.width == W + 4 and cache.lengths.tolist() == [W + 1, W + 4] and not cache.chunk and cache.n_new is None
        m._decoder()(_prompts(B, 3, 3), cache=cache)
        assert cache.width == W + 7 and cache.lengths.tolist() == [W + 4, W + 7]
        with pytest.raises(ValueError, match="full"):  # 13 + 4 > 16, whatever the rows' own lengths are
            cache.begin(B, 4)
        with pytest.raises(ValueError, match="truncate"):
            cache.truncate(torch.tensor((W, W)), W + 8)
        cache.truncate(torch.tensor((W + 1, W + 2)), W + 2)
        assert cache.width == W + 2 and cache.lengths.tolist() == [W + 1, W + 2] and cache.lengths.dtype == torch.int32
        assert cache.begin(B, 8) is False and cache.chunk  # fits again
        cache.advance(8)
        assert cache.width == 16 and cache.lengths.tolist() == [W + 9, W + 10]
        with pytest.raises(ValueError, match="full"):
            cache.begin(B, 1)


def test_chunk_past_the_cache_is_an_error_on_the_cpu():
    D, T = 64, 3
    q, k, v = cc.split_chunk(cc.append_inputs(D, T), D)
    kc, _ = cc.dc.guarded_cache(D, CPU)
    vc, _ = cc.dc.guarded_cache(D, CPU)
    pos = torch.tensor((0, cc.dc.APPEND_TMAX - T + 1, 0, 0), dtype=torch.int32)
    with pytest.raises(ValueError, match="KV cache"):
        fused.kv_append_chunk(q, k, v, pos, None, None, None, None, 0.0, kc, vc)
    fused.kv_append_chunk(q, k, v, pos, None, None, None, None, 0.0, kc, vc, torch.tensor((3, 2, 3, 3), dtype=torch.int32))


@pytest.mark.parametrize("D", cc.DIMS)
def test_pytorch_chunk_attention_meets_the_gpu_bound(D):
    fn = fused.chunk_attention_reference
    for T in (1, 5):
        cc.check_attention_case(fn, CPU, D, 8, 2, T, cc.length_sets(2, T)[0], splits=(None,))
    cc.check_attention_case(fn, CPU, D, 7, 1, 8, cc.length_sets(1, 8)[1], n_new=cc.ragged(8), splits=(None,))
    cc.check_attention_case(fn, CPU, D, 4, 4, 5, cc.WINDOW_CASES[1][1], window=16, splits=(None,), shared_cache=True)
    cc.check_attention_case(fn, CPU, D, 4, 4, 5, cc.WINDOW_CASES[0][1], n_new=cc.ragged(5), window=1, splits=(None,))
    for lens, max_len in cc.BOUND_CASES:
        cc.check_attention_case(fn, CPU, D, 8, 2, 5, lens, max_len=max_len, splits=(None,))


@pytest.mark.parametrize("mode", cc.MODES)
@pytest.mark.parametrize("D", cc.DIMS)
def test_pytorch_kv_append_chunk_is_bit_equal(D, mode):
    for T in (1, 3, 8):
        cc.check_append_chunk(fused.kv_append_chunk_reference, CPU, D, T, mode)
