"""Beam search on the CPU, in fp32 through the PyTorch forms: ``generate(num_beams=n)`` returns the sequences and
scores of transformers' ``generate`` on the stock classes (free and with an EOS, ragged prompts, every length
penalty / early-stopping combination), equals a naive beam search without a cache for every native family, needs
the cache reorder (negative control), leaves ``num_beams=1`` as it was; KVCache.repeat_rows / reorder_rows; the
argument refusals; generate.py's flags; and the bf16 twin of the GPU test's score check."""
import tempfile

import pytest
import torch
import transformers

import test_generate_gpu as tg
from beam_cases import naive_beam_search, score_ratio
from distributed_lion_pytorch_amd.models import KVCache
from test_generate_cpu import FAMILIES, _build, _prompts, model_of, naive_greedy

CPU = torch.device("cpu")
PAD = 3  # transformers fills with `pad_token_id or eos_token_id`: a pad id of 0 would not be used
_HF = {}


def hf_pair(family):
    if family not in _HF:
        m = _build(family, seed=2)
        with tempfile.TemporaryDirectory() as d:
            m.save_pretrained(d)
            cls = transformers.GPT2LMHeadModel if family == "gpt2" else transformers.LlamaForCausalLM
            hf = cls.from_pretrained(d).eval()
        hf.generation_config.eos_token_id = None
        _HF[family] = (m, hf)
    return _HF[family]


def _ragged(model, T=10, lens=(6, 10), seed=4):
    ids = _prompts(model, len(lens), T, seed=seed)
    mask = torch.ones_like(ids)
    for b, k in enumerate(lens):
        mask[b, :T - k] = 0
        ids[b, :T - k] = PAD
    return ids, mask


def _hf_generate(hf, ids, mask, n, eos=None, **kw):
    extra = dict(min_new_tokens=n) if eos is None else dict(eos_token_id=eos)
    with torch.no_grad():
        return hf.generate(ids, attention_mask=mask, do_sample=False, max_new_tokens=n, pad_token_id=PAD,
                           output_scores=True, return_dict_in_generate=True, **extra, **kw)


@pytest.mark.parametrize("num_beams", [2, 4])
@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_same_beams_as_hf_generate(family, num_beams):
    m, hf = hf_pair(family)
    ids, mask = _ragged(m)
    n, T = 8, ids.shape[1]
    finished_early, worst = 0, 0.0
    for n_ret in (1, num_beams):
        for lp in (1.0, 0.6, 2.0):
            for early in (False, True):
                kw = dict(num_beams=num_beams, num_return_sequences=n_ret, length_penalty=lp, early_stopping=early)
                name = f"{family} {kw}"
                ref = _hf_generate(hf, ids, mask, n, **kw)
                out = m.generate(ids, attention_mask=mask, max_new_tokens=n, return_dict_in_generate=True, **kw)
                assert torch.equal(out.sequences, ref.sequences), (name, out.sequences[:, T:], ref.sequences[:, T:])
                worst = max(worst, float((out.sequences_scores - ref.sequences_scores).abs().max()))
                assert float((out.sequences_scores - ref.sequences_scores).abs().max()) <= 1e-5, name
                assert out.sequences.shape == (2 * n_ret, T + n)
                # an EOS from the free run: the best beam of row 0 stops at its third token
                eos = int(ref.sequences[0, T + 2])
                ref = _hf_generate(hf, ids, mask, n, eos=eos, **kw)
                out = m.generate(ids, attention_mask=mask, max_new_tokens=n, eos_token_id=eos, pad_token_id=PAD,
                                 return_dict_in_generate=True, **kw)
                assert torch.equal(out.sequences, ref.sequences), (name, eos, out.sequences[:, T:], ref.sequences[:, T:])
                worst = max(worst, float((out.sequences_scores - ref.sequences_scores).abs().max()))
                assert float((out.sequences_scores - ref.sequences_scores).abs().max()) <= 1e-5, (name, eos)
                new = out.sequences[:, T:]
                finished_early += int(((new == eos).any(1) & (new[:, -1] != eos)).sum()) + int(new.shape[1] < n)
                plain = m.generate(ids, attention_mask=mask, max_new_tokens=n, eos_token_id=eos, pad_token_id=PAD, **kw)
                assert torch.equal(plain, out.sequences)
    print(f"[beam] {family} {num_beams} beams: max |sequences_scores - HF's| = {worst:.2e}; {finished_early} returned "
          f"beams ended before the last step")
    assert finished_early > 0, "no beam finished before the last step: the EOS cases tested nothing"


@pytest.mark.parametrize("family", FAMILIES)
def test_beam_search_equals_the_naive_loop(family):
    m = model_of(family)
    ids = _prompts(m, 2, 12, seed=8)
    for kw in (dict(nb=3, n_ret=3), dict(nb=2, n_ret=1, length_penalty=0.6, early_stopping=True)):
        free, _ = naive_beam_search(m, ids, 10, **kw)
        for eos in (None, int(free[0, 12 + 3])):
            ref, ref_scores = naive_beam_search(m, ids, 10, eos=eos, pad=PAD, **kw)
            out = m.generate(ids, max_new_tokens=10, num_beams=kw["nb"], num_return_sequences=kw["n_ret"],
                             length_penalty=kw.get("length_penalty", 1.0), early_stopping=kw.get("early_stopping", False),
                             eos_token_id=eos, pad_token_id=PAD, return_dict_in_generate=True)
            assert torch.equal(out.sequences, ref), (family, kw, eos, out.sequences[:, 12:], ref[:, 12:])
            assert float((out.sequences_scores - ref_scores).abs().max()) <= 1e-5


def test_without_the_cache_reorder_the_result_differs(monkeypatch):
    """Negative control: the beams of this case cross, and a cache that is not reordered gives other beams than
    transformers does."""
    m, hf = hf_pair("llama")
    ids, mask = _ragged(m)
    kw = dict(num_beams=4, num_return_sequences=4)
    ref = _hf_generate(hf, ids, mask, 8, **kw)
    seen = []
    real = KVCache.reorder_rows
    monkeypatch.setattr(KVCache, "reorder_rows", lambda self, index, lo=0: (seen.append(index.clone()), real(self, index, lo))[1])
    out = m.generate(ids, attention_mask=mask, max_new_tokens=8, **kw)
    assert torch.equal(out, ref.sequences)
    straight = torch.arange(8)
    assert len(seen) == 7 and any(not torch.equal(i, straight) for i in seen), "the beams never crossed"
    monkeypatch.setattr(KVCache, "reorder_rows", lambda self, index, lo=0: None)
    broken = m.generate(ids, attention_mask=mask, max_new_tokens=8, **kw)
    assert broken.shape == ref.sequences.shape and not torch.equal(broken, ref.sequences)


def test_repeat_rows_and_reorder_rows():
    m = model_of("llama")
    cache = KVCache(m.config, 2, 12, CPU, torch.float32)
    g = torch.Generator().manual_seed(0)
    cache._buf.copy_(torch.randn(cache._buf.shape, generator=g))
    cache.width, cache.prefilled = 5, True
    cache.set_lengths(torch.tensor([3, 5]))
    big = cache.repeat_rows(3)
    assert big.batch == 6 and big.max_len == 12 and big.width == 5 and big.prefilled
    assert big.lengths.tolist() == [3, 3, 3, 5, 5, 5] and big.lengths.dtype == torch.int32
    for r in range(6):
        assert torch.equal(big._buf[:, :, r, :5], cache._buf[:, :, r // 3, :5])
    assert float(big._buf[:, :, :, 5:].abs().max()) == 0.0, "positions at and beyond width are not copied"
    assert big.layer(1)[0].shape == (6, 12) + cache.layer(1)[0].shape[2:]
    big._buf.copy_(torch.randn(big._buf.shape, generator=g))
    big.lengths.copy_(torch.tensor([4, 5, 6, 7, 8, 9]))
    big.width = 9
    before = big._buf.clone()
    index = torch.tensor([2, 0, 0, 5, 5, 3])
    big.reorder_rows(index, lo=4)
    assert big.lengths.tolist() == [6, 4, 4, 9, 9, 7]
    assert torch.equal(big._buf[:, :, :, 4:9], before[:, :, index, 4:9])
    assert torch.equal(big._buf[:, :, :, :4], before[:, :, :, :4]), "below lo nothing moves"
    assert torch.equal(big._buf[:, :, :, 9:], before[:, :, :, 9:]), "at and beyond width nothing moves"
    big.reorder_rows(torch.tensor([1, 0, 2, 3, 4, 5]), lo=9)  # lo == width: lengths only
    assert torch.equal(big._buf, torch.cat([before[:, :, :, :4], before[:, :, index, 4:9], before[:, :, :, 9:]], dim=3))
    assert big.lengths.tolist() == [4, 6, 4, 9, 9, 7]


def test_argument_refusals():
    m = model_of("llama")
    ids = _prompts(m, 2, 6)
    for match, kw in [("do_sample", dict(num_beams=2, do_sample=True)),
                      ("num_return_sequences", dict(num_beams=2, num_return_sequences=3)),
                      ("num_return_sequences", dict(num_return_sequences=2)),
                      ("early_stopping", dict(num_beams=2, early_stopping="never")),
                      ("num_beams", dict(num_beams=33)),  # 66 candidates per beam: beyond the kernel's k
                      ("num_beams", dict(num_beams=12, eos_token_id=[1, 2, 3, 4, 5])),  # 72
                      ("num_beams", dict(num_beams=0))]:
        with pytest.raises(ValueError, match=match):
            m.generate(ids, max_new_tokens=2, **kw)
    small = tg.L.LlamaForCausalLM(tg.L.llama_config("llama-tiny", vocab_size=40)).eval()
    with pytest.raises(ValueError, match="num_beams"):
        small.generate(ids % 40, max_new_tokens=2, num_beams=21)  # 42 candidates from a vocabulary of 40
    assert small.generate(ids % 40, max_new_tokens=2, num_beams=20, num_return_sequences=20).shape == (40, 8)


@pytest.mark.parametrize("family", ["gpt2", "qwen2"])
def test_one_beam_is_greedy_as_before(family):
    m = model_of(family)
    ids = _prompts(m, 3, 12)
    ref, _ = naive_greedy(m, ids, 10)
    out = m.generate(ids, max_new_tokens=10, num_beams=1, num_return_sequences=1, length_penalty=2.0, early_stopping=True)
    assert torch.equal(out, ref)
    full = m.generate(ids, max_new_tokens=10, return_dict_in_generate=True)
    assert torch.equal(full.sequences, ref) and full.sequences_scores is None
    a = m.generate(ids, max_new_tokens=6, do_sample=True, top_k=5, seed=3)
    assert torch.equal(a, m.generate(ids, None, 6, True, 1.0, 5, 1.0, None, None, 3))  # positional calls as before


def test_generate_py_beam_flags(capsys):
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import generate

    out = generate.main(["--model_name_or_path", "gpt2-tiny", "--config_overrides", "n_layer=1,n_embd=32,n_head=2",
                         "--prompt", "ab", "--prompt", "abcd", "--max_new_tokens", "5", "--device", "cpu",
                         "--num_beams", "3", "--num_return_sequences", "2", "--length_penalty", "0.8",
                         "--early_stopping"])
    assert out.shape[0] == 4 and out.shape[1] <= 4 + 5
    text = capsys.readouterr().out
    assert text.count("--- 'ab' [beam ") == 2 and text.count("--- 'abcd' [beam ") == 2


@pytest.mark.parametrize("family", ["gpt2", "llama", "mistral"])
def test_bf16_score_check_is_reachable_by_the_pytorch_forms(family):
    """The condition of tests/test_beam_search_gpu.py on the CPU: the bf16 model through the PyTorch forms against
    its fp32 twin."""
    torch.manual_seed(0)
    m32 = tg._build(family)
    m16 = tg._build(family)
    m16.load_state_dict(m32.state_dict())
    m16 = m16.to(torch.bfloat16)
    m32.load_state_dict({k: v.float() for k, v in m16.state_dict().items()})
    ids, mask = tg_prompts(CPU)
    out = m16.generate(ids, attention_mask=mask, max_new_tokens=12, num_beams=4, num_return_sequences=4,
                       return_dict_in_generate=True)
    ratio = score_ratio(m16, m32, ids, mask, out.sequences, out.sequences_scores, 4, None, 1.0)
    print(f"[beam] {family} (PyTorch forms, bf16): |S - sum l32| / sum |l16 - l32| = {ratio:.3f}")
    assert ratio <= tg.MAX_RATIO


def tg_prompts(device, B=2, T=40, lens=(17, 33), seed=21):
    """Ragged prompts of the GPU cases: row 0 left-padded, the others right-padded."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 256, (B, T), generator=g)
    mask = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        k = lens[b % len(lens)]
        mask[b, T - k:] = 1 if b == 0 else 0
        if b:
            mask[b, :k] = 1
    return ids.to(device), mask.to(device)
