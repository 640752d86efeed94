"""The extend path on the CPU through the PyTorch forms: fused.extend_attention meets the GPU tests' bound on their
cases (tests/chunk_cases.py); in fp32, forwards of 11 tokens per row on the cache (extend=True) equal the full
forward, and generate(prefill_chunk_size=...) equals generate() token for token."""
import pytest
import torch

import chunk_cases as cc
from distributed_lion_pytorch_amd.models import KVCache
from distributed_lion_pytorch_amd.ops import fused
from test_speculative_cpu import _CLI, CPU, FAMILIES, _prompts, model_of


@pytest.mark.parametrize("D", cc.DIMS)
def test_pytorch_form_meets_the_gpu_bound(D):
    fn, one = fused.extend_attention, (None,)
    for T in (9, fused.EXTEND_TQ + 1):
        cc.check_attention_case(fn, CPU, D, 8, 2, T, (0, 64 - T, cc.TMAX - T), splits=one)
    cc.check_attention_case(fn, CPU, D, 7, 1, 17, (140, 300, 1), n_new=cc.ragged(17), splits=one)
    cc.check_attention_case(fn, CPU, D, 4, 4, 17, cc.WINDOW_CASES[1][1], window=16, splits=one, shared_cache=True)
    for lens, max_len in cc.BOUND_CASES:
        cc.check_attention_case(fn, CPU, D, 8, 2, 17, lens, max_len=max_len, splits=one)


@pytest.mark.parametrize("family", FAMILIES)
def test_extend_forwards_equal_the_full_forward(family):
    m = model_of(family)
    B, SEQ, PIECE = 3, 40, 11
    lens = torch.tensor((3, 7, 5))
    W = int(lens.max())
    steps = -(-(SEQ - int(lens.min())) // PIECE)
    seq = _prompts(B, SEQ, seed=5)
    rows, t = torch.arange(B), torch.arange(PIECE)
    cache = KVCache(m.config, B, W + steps * PIECE, CPU, torch.float32)
    with torch.no_grad():
        full = m(seq).logits
        prompt = torch.where(torch.arange(W)[None] < lens[:, None], seq[:, :W], torch.zeros_like(seq[:, :W]))
        got = m(prompt, cache=cache).logits[rows, lens - 1]
        assert torch.allclose(got, full[rows, lens - 1], rtol=1e-5, atol=1e-5)
        cache.set_lengths(lens)
        with pytest.raises(ValueError, match="1 to 8"):
            cache.begin(B, PIECE)
        for s in range(steps):
            pos = lens[:, None] + s * PIECE + t[None, :]
            live = pos < SEQ
            out = m(seq.gather(1, pos.clamp_max(SEQ - 1)), cache=cache, n_new=live.sum(1).to(torch.int32), extend=True).logits
            want = full[rows[:, None].expand_as(pos)[live], pos[live]]
            assert torch.allclose(out[live], want, rtol=1e-5, atol=1e-5), (family, s, float((out[live] - want).abs().max()))
    assert cache.lengths.tolist() == [SEQ] * B and cache.width == W + steps * PIECE


@pytest.mark.parametrize("family", FAMILIES)
def test_chunked_prefill_generates_the_same_tokens(family):
    m = model_of(family)
    ids = _prompts(3, 17, seed=4)
    mask = torch.ones_like(ids)
    mask[0, :9] = 0  # left-padded rows: one ends inside the first piece's successor, one is full width
    mask[2, :3] = 0
    for kw in (dict(), dict(num_beams=3, num_return_sequences=2), dict(do_sample=True, seed=3, top_k=20)):
        plain = m.generate(ids, attention_mask=mask, max_new_tokens=8, **kw)
        for n in (5, 16, 17):
            got = m.generate(ids, attention_mask=mask, max_new_tokens=8, prefill_chunk_size=n, **kw)
            assert torch.equal(got, plain), (family, kw, n, got[:, 17:], plain[:, 17:])
    a = model_of(family, 1, 1)
    plain = m.generate(ids, attention_mask=mask, max_new_tokens=8)
    assert torch.equal(m.generate(ids, attention_mask=mask, max_new_tokens=8, assistant_model=a, prefill_chunk_size=5), plain)
    with pytest.raises(ValueError, match="prefill_chunk_size"):
        m.generate(ids, max_new_tokens=2, prefill_chunk_size=0)


def test_generate_py_prefill_chunk_size():
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import generate

    # an untrained gpt2-tiny has near-tied logits, so the tokens are compared on the margin-checked models above; here
    # the flag must reach generate(): a valid value runs, an invalid one is generate's own refusal
    plain, got = generate.main(_CLI), generate.main(_CLI + ["--prefill_chunk_size", "3"])
    assert got.shape[0] == 2 and torch.equal(got[:, :4], plain[:, :4])
    with pytest.raises(ValueError, match="prefill_chunk_size must be >= 1"):
        generate.main(_CLI + ["--prefill_chunk_size", "0"])
