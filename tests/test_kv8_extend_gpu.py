"""More than 8 tokens per row on an fp8 KV cache: fused.cached_attention_fp8 (csrc/kv8_extend_attention.hip) against
fp64 on the dequantised cache and the fp8 stores of fused.kv_append_chunk bit for bit, through the cases and checks of
tests/kv8_cases.py, and the extend forwards / chunked prefill of the tiny models of test_speculative_gpu.py under the
measure of test_kv8_gpu.test_layer0_bits_and_logits.  Every PyTorch form is patched to fail.
docs/TEST_TOLERANCES.md "FP8 KV cache" has the conditions and the measured figures."""
import pytest
import torch

import chunk_cases as cc
import kv8_cases as k8
import numerics as nm
import test_kv8_gpu as t8
from distributed_lion_pytorch_amd.models import KVCache
from distributed_lion_pytorch_amd.ops import fused, hip
from test_speculative_gpu import FAMILIES, LENS, SEQ, exact_logits, pair

pytestmark = pytest.mark.gpu

SPLITS = (None, 1, 2, fused._EXTEND_MAX_SPLITS)
PIECE = 24  # tests/test_extend_gpu.py's schedule
# max over (row, position) of E_k / (E_q + E_f) on the extend schedule.  Measured 1.03 (gpt2), 1.02 (llama), 1.11
# (mistral), 1.22 (qwen3): the worst times 2, rounded up to a half, is test_kv8_gpu's 2.5
MAX_RATIO = t8.MAX_RATIO


def kernels_only(monkeypatch):
    t8.kernels_only(monkeypatch)
    monkeypatch.setattr(fused, "extend_attention_reference", lambda *a, **kw: pytest.fail("PyTorch extend_attention ran"))


def length_sets(Hkv, T):
    """test_extend_attention_gpu.length_sets: an empty cache, len + T on 63 / 64 / 65, on either side of the unforced
    grid's first split boundary, and a row that ends exactly at TMAX."""
    splits, c = fused.extend_splits(k8.B, Hkv, k8.TMAX, T)
    assert splits >= 2, "the cases are meant to cross a split boundary of the unforced grid"
    return [(0, 0, 0), (63 - T, 64 - T, 65 - T), (c - 1 - T, c - T, c + 1 - T), (k8.TMAX - T, 2 * c - T, 1)]


@pytest.mark.parametrize("T", (9, 16, 17, 33))
@pytest.mark.parametrize("H,Hkv", k8.HEADS)
@pytest.mark.parametrize("D", k8.DIMS)
def test_lengths_and_splits(D, H, Hkv, T, cuda, monkeypatch):
    hip.require()
    kernels_only(monkeypatch)
    worst = 0.0
    for lens in length_sets(Hkv, T):
        worst = max(worst, k8.check_attention_case(fused.cached_attention_fp8, cuda, D, H, Hkv, T, lens, splits=SPLITS))
    print(f"[kv8 extend] D={D} H={H}/{Hkv} T={T}: worst row ratio {worst:.3f} of C_ROWS = {nm.C_ROWS}")


@pytest.mark.parametrize("T", (9, 17, 33))
@pytest.mark.parametrize("H,Hkv", [(8, 2), (7, 1)])
@pytest.mark.parametrize("D", k8.DIMS)
def test_ragged_windows_and_bounds(D, H, Hkv, T, cuda, monkeypatch):
    hip.require()
    kernels_only(monkeypatch)
    fn = fused.cached_attention_fp8
    worst = k8.check_attention_case(fn, cuda, D, H, Hkv, T, length_sets(Hkv, T)[2], k8.ragged(T), splits=SPLITS)
    for window, lens in k8.WINDOW_CASES:
        worst = max(worst, k8.check_attention_case(fn, cuda, D, H, Hkv, T, lens, k8.ragged(T), window, splits=SPLITS))
    for lens, max_len in k8.BOUND_CASES:  # every len + T stays within TMAX for T <= 33
        worst = max(worst, k8.check_attention_case(fn, cuda, D, H, Hkv, T, lens, None, 0, splits=SPLITS, max_len=max_len))
    print(f"[kv8 extend] ragged / windows / bounds D={D} H={H}/{Hkv} T={T}: worst row ratio {worst:.3f}")


@pytest.mark.parametrize("mode", cc.MODES)
@pytest.mark.parametrize("T", (9, 17, 26))
@pytest.mark.parametrize("D", k8.DIMS)
def test_kv_append_chunk_fp8_above_8_tokens(D, T, mode, cuda, monkeypatch):
    hip.require()
    kernels_only(monkeypatch)
    k8.check_append_chunk(fused.kv_append_chunk, cuda, D, T, mode)
    fused.check_index_errors(blocking=True)


def extend_forced(m, seq, lens, kv_dtype):
    """Logits [B, SEQ, V] (NaN where not computed) and the cache of test_extend_gpu's schedule: a prefill of max(LENS)
    columns, then extend forwards of PIECE tokens per row, ragged where a row runs out of tokens."""
    B, dev = seq.shape[0], seq.device
    W, steps = max(LENS), -(-(SEQ - min(LENS)) // PIECE)
    rows, t = torch.arange(B, device=dev), torch.arange(PIECE, device=dev)
    cache = KVCache(m.config, B, W + (steps + 1) * PIECE, dev, m.lm_head.weight.dtype, kv_dtype)
    out = torch.full((B, SEQ, m.config.vocab_size), float("nan"), device=dev)
    with torch.no_grad():
        prompt = torch.where(torch.arange(W, device=dev)[None] < lens[:, None], seq[:, :W], torch.zeros_like(seq[:, :W]))
        out[rows, lens - 1] = m(prompt, cache=cache).logits[rows, lens - 1].float()
        cache.set_lengths(lens)
        for s in range(steps):
            first = lens + s * PIECE
            pos = first[:, None] + t[None, :]
            n_new = (SEQ - first).clamp(0, PIECE)
            live = t[None, :] < n_new[:, None]
            logits = m(seq.gather(1, pos.clamp_max(SEQ - 1)), cache=cache, n_new=n_new.to(torch.int32), extend=True).logits
            out[rows[:, None].expand_as(pos)[live], pos[live]] = logits.float()[live]
    return out, cache


@pytest.mark.parametrize("family", FAMILIES)
def test_models_extend_and_chunked_prefill(family, cuda, monkeypatch):
    hip.require()
    m, ref = pair(family, cuda)
    seq = torch.randint(1, 256, (3, SEQ), generator=torch.Generator().manual_seed(9)).to(cuda)
    lens = torch.tensor(LENS, device=cuda)
    exact = exact_logits(ref, seq)
    with torch.no_grad():
        full = m(seq).logits.float()
    fused.set_impl("torch")
    try:
        twin8, _ = extend_forced(ref, seq, lens, "fp8_e4m3")  # the fp32 twin on an fp8 cache: quantisation alone
    finally:
        fused.set_impl("auto")
    _, cache16 = extend_forced(m, seq, lens, None)
    kernels_only(monkeypatch)
    got, cache8 = extend_forced(m, seq, lens, "fp8_e4m3")
    assert cache8.lengths.tolist() == [SEQ] * 3 and cache16.lengths.tolist() == [SEQ] * 3
    for j, what in enumerate(("keys", "values")):
        ec, es = fused.kv_quantize_reference(cache16.layer(0)[j][:, :SEQ])
        nm.assert_bits(cache8.layer(0)[j][:, :SEQ], ec, f"{family}: layer 0 {what}, codes")
        nm.assert_bits(cache8.layer_scales(0)[j][:, :SEQ], es, f"{family}: layer 0 {what}, scales")
    done = ~torch.isnan(got).any(-1)
    assert bool((done == (torch.arange(SEQ, device=cuda)[None] >= (lens - 1)[:, None])).all())
    err = lambda x: torch.where(done, (torch.nan_to_num(x) - exact).abs().amax(-1), torch.zeros_like(exact[..., 0]))
    e_k, e_q, e_f = err(got), err(twin8), err(full)
    ratio = torch.where(done, e_k / (e_q + e_f), torch.zeros_like(e_k))
    print(f"[kv8 extend] {family}: E_k / (E_q + E_f) max {float(ratio.max()):.3f}, median {float(ratio[done].median()):.3f}")
    assert float(ratio.max()) <= MAX_RATIO
    # a chunked prefill on the fp8 cache: pieces of 16, 16 and 9 columns, the first of them the flash forward
    ids = torch.randint(1, 256, (3, 41), generator=torch.Generator().manual_seed(13)).to(cuda)
    mask = torch.ones_like(ids)
    mask[0, :7] = 0
    kw = dict(attention_mask=mask, max_new_tokens=12, kv_cache_dtype="fp8_e4m3", prefill_chunk_size=16)
    out = m.generate(ids, **kw)
    assert out.shape == (3, 53) and torch.equal(out[:, :41], ids)
    assert torch.equal(m.generate(ids, **kw), out)
    fused.check_index_errors(blocking=True)
