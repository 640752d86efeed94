"""``generate(num_beams=n, beam_cache="shared")`` on the CPU, in fp32 through the PyTorch forms: the sequences of the
default (repeated) cache and its scores within the 1e-5 of tests/test_beam_search_cpu.py, for ragged left- and
right-padded prompts and a prefill in pieces; the refusals; generate.py's flag."""
import pytest
import torch

from distributed_lion_pytorch_amd.models.generation import BeamKVCache, KVCache
from test_beam_search_cpu import PAD, _ragged, tg_prompts
from test_generate_cpu import _prompts, model_of

FAMILIES = ["gpt2", "llama", "mistral", "qwen3"]  # mistral: a window of 8 that cuts inside the prompt


@pytest.mark.parametrize("piece", [None, 4])
@pytest.mark.parametrize("family", FAMILIES)
def test_shared_cache_gives_the_default_beams(family, piece, monkeypatch):
    m = model_of(family)
    left = _ragged(m)  # left-padded, lengths 6 and 10
    ids, mask = tg_prompts(torch.device("cpu"), T=10, lens=(5, 9))  # row 0 left-padded, row 1 right-padded
    made = []
    real = BeamKVCache.__init__
    monkeypatch.setattr(BeamKVCache, "__init__", lambda self, *a, **kw: (made.append(self), real(self, *a, **kw))[1])
    for ids, mask in (left, (ids % m.config.vocab_size, mask)):
        free = m.generate(ids, attention_mask=mask, max_new_tokens=8, num_beams=3)
        for eos in (None, int(free[0, 10 + 2])):
            kw = dict(attention_mask=mask, max_new_tokens=8, num_beams=3, num_return_sequences=3, eos_token_id=eos,
                      pad_token_id=PAD, length_penalty=0.8, prefill_chunk_size=piece, return_dict_in_generate=True)
            ref = m.generate(ids, **kw)
            out = m.generate(ids, beam_cache="shared", **kw)
            assert torch.equal(out.sequences, ref.sequences), (family, eos)
            assert float((out.sequences_scores - ref.sequences_scores).abs().max()) <= 1e-5
    assert len(made) == 4, "the shared path builds one BeamKVCache per call"
    assert made[0].prefix.max_len == 10 and made[0].suffix.batch == 6 and made[0].suffix.max_len == 8


def test_refusals_and_protocol():
    m = model_of("llama")
    ids = _prompts(m, 2, 6)
    group = m.config.num_attention_heads // m.config.num_key_value_heads
    for match, kw in [("num_beams > 1", dict(beam_cache="shared")),
                      ("kv_cache_dtype", dict(beam_cache="shared", num_beams=2, kv_cache_dtype="fp8_e4m3")),
                      ("<= 64", dict(beam_cache="shared", num_beams=64 // group + 1)),
                      ("beam_cache", dict(beam_cache="paged", num_beams=2))]:
        with pytest.raises(ValueError, match=match):
            m.generate(ids, max_new_tokens=2, **kw)
    prefix = KVCache(m.config, 2, 6)
    with pytest.raises(ValueError, match="prefilled"):
        BeamKVCache(prefix, 2, 4, m.config)
    with torch.no_grad():
        m.model(ids, cache=prefix)
        cache = BeamKVCache(prefix, 2, 4, m.config)
        for bad in (dict(T=2), dict(T=1, extend=True), dict(T=1, n_new=torch.ones(4, dtype=torch.int32))):
            with pytest.raises(ValueError, match="one token"):
                cache.begin(4, **bad)
        m.model(ids.repeat_interleave(2, 0)[:, :1], cache=cache)
    assert cache.positions.tolist() == [6] * 4 and cache.suffix.lengths.tolist() == [1] * 4 and cache.max_len == 10


def test_generate_py_beam_cache_flag(capsys):
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import generate

    argv = ["--model_name_or_path", "gpt2-tiny", "--config_overrides", "n_layer=1,n_embd=32,n_head=2", "--prompt", "ab",
            "--prompt", "abcd", "--max_new_tokens", "5", "--device", "cpu", "--num_beams", "3", "--num_return_sequences", "2"]
    torch.manual_seed(0)  # the named size is initialised at random
    ref = generate.main(argv)
    torch.manual_seed(0)
    out = generate.main(argv + ["--beam_cache", "shared"])
    assert torch.equal(out, ref)
    assert capsys.readouterr().out.count("--- 'abcd' [beam ") == 4
