"""Forwards of more than 8 tokens per row on the cache (extend=True: fused.kv_append_chunk + csrc/extend_attention.hip)
on the GPU in bf16, with the tiny kernel-eligible models, the fp32 twins and the conditions of
tests/test_speculative_gpu.py: the extend path's logit error against the fp32 twin is at most MAX_RATIO times the full
bf16 forward's; generate(prefill_chunk_size=...) equals generate() wherever the fp32 twin's argmax is decided."""
import pytest
import torch

import test_speculative_gpu as sg
from distributed_lion_pytorch_amd.models import KVCache
from distributed_lion_pytorch_amd.ops import fused, hip

pytestmark = pytest.mark.gpu

PIECE = 24


def kernels_only(monkeypatch):
    sg.kernels_only(monkeypatch)
    monkeypatch.setattr(fused, "extend_attention_reference", lambda *a, **kw: pytest.fail("PyTorch extend_attention ran"))


def ratio_to_full(cached, done, full, exact):
    e_full = (full - exact).abs().amax(-1)
    e_cached = torch.where(done, (torch.nan_to_num(cached) - exact).abs().amax(-1), torch.zeros_like(e_full))
    return torch.where(done, e_cached / e_full, torch.zeros_like(e_full))


@pytest.mark.parametrize("family", sg.FAMILIES)
def test_extend_teacher_forced_consistency_and_rollback(family, cuda, monkeypatch):
    hip.require()
    m, ref = sg.pair(family, cuda)
    SEQ, B = sg.SEQ, 3
    seq = torch.randint(1, 256, (B, SEQ), generator=torch.Generator().manual_seed(9)).to(cuda)
    lens = torch.tensor(sg.LENS, device=cuda)
    exact = sg.exact_logits(ref, seq)
    with torch.no_grad():
        full = m(seq).logits.float()
    kernels_only(monkeypatch)
    W, steps = max(sg.LENS), -(-(SEQ - min(sg.LENS)) // PIECE)
    rows, t = torch.arange(B, device=cuda), torch.arange(PIECE, device=cuda)
    cache = KVCache(m.config, B, W + (steps + 1) * PIECE, cuda, m.lm_head.weight.dtype)
    cached = torch.full_like(full, float("nan"))

    def extend(first, n_new):
        """One forward of PIECE tokens per row from position first[b] on, of which row b keeps n_new[b]."""
        pos = first[:, None] + t[None, :]
        live = t[None, :] < n_new[:, None]
        logits = m(seq.gather(1, pos.clamp_max(SEQ - 1)), cache=cache, n_new=n_new.to(torch.int32), extend=True).logits.float()
        cached[rows[:, None].expand_as(pos)[live], pos[live]] = logits[live]

    with torch.no_grad():
        prompt = torch.where(torch.arange(W, device=cuda)[None] < lens[:, None], seq[:, :W], torch.zeros_like(seq[:, :W]))
        cached[rows, lens - 1] = m(prompt, cache=cache).logits[rows, lens - 1].float()
        cache.set_lengths(lens)
        with pytest.raises(ValueError, match="1 to 8"):
            cache.begin(B, 9)
        for s in range(steps):
            first = lens + s * PIECE
            extend(first, (SEQ - first).clamp(0, PIECE))
    done = ~torch.isnan(cached).any(-1)
    assert bool((done == (torch.arange(SEQ, device=cuda)[None] >= (lens - 1)[:, None])).all())
    assert cache.lengths.tolist() == [SEQ] * B and cache.width == W + steps * PIECE
    ratio = ratio_to_full(cached, done, full, exact)
    print(f"[extend] {family}: extend / full logit error against fp32, max ratio {float(ratio.max()):.3f}, median "
          f"{float(ratio[done].median()):.3f}")
    assert float(ratio.max()) <= sg.MAX_RATIO
    # rollback: two rows lose their last 20 tokens and take them again in one forward
    keep = torch.tensor((SEQ - 20, SEQ, SEQ - 20), device=cuda)
    cache.truncate(keep, SEQ)
    cached[:, SEQ - 20:] = float("nan")
    with torch.no_grad():
        extend(keep, SEQ - keep)
    assert cache.lengths.tolist() == [SEQ] * B and cache.width == SEQ + PIECE
    again = ~torch.isnan(cached).any(-1)
    assert again[0, SEQ - 20:].all() and again[2, SEQ - 20:].all() and not again[1, SEQ - 20:].any()
    assert float(ratio_to_full(cached, again, full, exact).max()) <= sg.MAX_RATIO
    fused.check_index_errors(blocking=True)


@pytest.mark.parametrize("family", sg.FAMILIES)
def test_chunked_prefill_equals_plain_greedy_where_decided(family, cuda, monkeypatch):
    hip.require()
    m, _ = sg.target(family, cuda)
    ids, mask, free, prefix = sg.plain_run(family, cuda)
    assert min(prefix) >= sg.MIN_PREFIX, f"{family}: compared prefix {prefix}"
    kernels_only(monkeypatch)
    out = m.generate(ids, attention_mask=mask, max_new_tokens=sg.NEW, prefill_chunk_size=16)
    assert out.shape == free.shape
    sg.assert_same_where_decided(out, free, prefix, f"{family} / prefill_chunk_size=16")
    with pytest.raises(ValueError, match="prefill_chunk_size"):
        m.generate(ids, max_new_tokens=2, prefill_chunk_size=0)
    fused.check_index_errors(blocking=True)
