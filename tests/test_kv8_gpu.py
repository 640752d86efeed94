"""The fp8 KV cache on the GPU: the quantising writers (kv_quantize, the fp8 stores of kv_append / kv_append_chunk)
bit for bit against fused.kv_quantize_reference, cached_attention_fp8 (csrc/kv8_attention.hip) against fp64 on the
dequantised cache, and the cached forwards / generate of the tiny kernel-eligible models of test_speculative_gpu.py.
docs/TEST_TOLERANCES.md "FP8 KV cache" has the conditions and the measured figures."""
import pytest
import torch

import chunk_cases as cc
import decode_cases as dc
import kv8_cases as k8
import numerics as nm
from distributed_lion_pytorch_amd.models import KVCache
from distributed_lion_pytorch_amd.ops import fused, hip
from test_speculative_gpu import CHUNK, FAMILIES, LENS, SEQ, exact_logits, pair

pytestmark = pytest.mark.gpu

# max over (row, position) of E_k / (E_q + E_f): the bf16 kernel path on an fp8 cache against the fp32 twin's
# quantisation error plus the full bf16 forward's error.  Measured 1.03 (gpt2), 1.06 (llama), 1.14 (mistral), 1.24
# (qwen3): the worst times a margin of 2, rounded up to a half (docs/TEST_TOLERANCES.md "FP8 KV cache")
MAX_RATIO = 2.5


def kernels_only(monkeypatch):
    for name in ("decode_attention_reference", "kv_append_reference", "chunk_attention_reference",
                 "kv_append_chunk_reference", "cached_attention_fp8_reference"):
        monkeypatch.setattr(fused, name, lambda *a, _n=name, **kw: pytest.fail(f"PyTorch {_n} ran"))


# ------------------------------------------------------------------------------------------- quantiser bits
@pytest.mark.parametrize("D", dc.DIMS)
def test_kv_quantize_bits(D, cuda):
    hip.require()
    g = torch.Generator().manual_seed(D)
    rows = torch.stack(list(k8.hand_rows().values()))  # [n, 64]
    x = torch.randn(3, 37, 2, D, generator=g) * torch.exp2(torch.randint(-20, 20, (3, 37, 2, 1), generator=g))
    x[0, :rows.shape[0], 0, :64] = rows.float()
    x[1, :rows.shape[0], 1, D - 64:] = rows.float()
    packed = torch.cat([torch.zeros(3, 37, 3 * D), x.reshape(3, 37, 2 * D)], dim=-1).to(torch.bfloat16).to(cuda)
    view = packed[..., 3 * D:].view(3, 37, 2, D)  # a column view of a wider projection output
    assert not view.is_contiguous()
    n = 3 * 40 * 2
    cbuf = torch.full((n * D + 2 * dc.GUARD,), k8.POISON_CODE, dtype=torch.uint8, device=cuda)
    sbuf = torch.full((n + 2 * dc.GUARD,), k8.POISON_SCALE, dtype=torch.float32, device=cuda)
    codes, scales = cbuf[dc.GUARD:dc.GUARD + n * D].view(3, 40, 2, D), sbuf[dc.GUARD:dc.GUARD + n].view(3, 40, 2)
    fused.kv_quantize(view, codes, scales)
    written = torch.zeros(3, 40, dtype=torch.bool, device=cuda)
    written[:, :37] = True
    k8.assert_cache8(f"kv_quantize D={D}", codes, scales, cbuf, sbuf, written, view.reshape(-1, 2, D))
    ec, es = fused.kv_quantize_reference(view.cpu())  # torch's CPU cast is the arbiter
    nm.assert_bits(codes[:, :37].cpu(), ec, "kv_quantize against the CPU cast, codes")
    nm.assert_bits(scales[:, :37].cpu(), es, "kv_quantize against the CPU cast, scales")


@pytest.mark.parametrize("mode", cc.MODES)
@pytest.mark.parametrize("D", dc.DIMS)
def test_kv_append_fp8_bits(D, mode, cuda, monkeypatch):
    hip.require()
    monkeypatch.setattr(fused, "kv_append_reference", lambda *a, **kw: pytest.fail("PyTorch kv_append ran"))
    k8.check_append(fused.kv_append, cuda, D, mode)
    fused.check_index_errors(blocking=True)


@pytest.mark.parametrize("mode", cc.MODES)
@pytest.mark.parametrize("D", dc.DIMS)
def test_kv_append_chunk_fp8_bits(D, mode, cuda, monkeypatch):
    hip.require()
    monkeypatch.setattr(fused, "kv_append_chunk_reference", lambda *a, **kw: pytest.fail("PyTorch kv_append_chunk ran"))
    for T in (1, 5, 8):
        k8.check_append_chunk(fused.kv_append_chunk, cuda, D, T, mode)
    fused.check_index_errors(blocking=True)


@pytest.mark.parametrize("mode", cc.MODES)
def test_one_key_three_writers(mode, cuda):
    """The same token at the same position through the prefill's kv_quantize (of fused.rope / qk_norm_rope), a decode
    step and a chunk: the same cached bits."""
    hip.require()
    D, pos = 128, 7
    cos, sin, gq, gk = k8.append_args(D, mode, cuda)
    q, k, v = dc.split_step(dc.append_inputs(D)[0].to(cuda), D)
    p = torch.full((dc.APPEND_B,), pos, dtype=torch.int32, device=cuda)
    got = []
    for writer in ("prefill", "step", "chunk"):
        kc, ks, _, _ = k8.guarded_cache8(D, cuda)
        vc, vs, _, _ = k8.guarded_cache8(D, cuda)
        if writer == "prefill":
            full = torch.zeros(dc.APPEND_B, dc.APPEND_TMAX, dc.APPEND_HKV, D, dtype=torch.bfloat16, device=cuda)
            full[:, pos] = k
            if mode != "append":
                full = fused.rope(full, cos, sin) if gk is None else fused.qk_norm_rope(full, gk, dc.APPEND_EPS, cos, sin)
            fused.kv_quantize(full, kc, ks)
            fused.kv_quantize(v[:, None].expand(-1, dc.APPEND_TMAX, -1, -1), vc, vs)
        elif writer == "step":
            fused.kv_append(q, k, v, p, cos, sin, gq, gk, dc.APPEND_EPS, kc, vc, ks, vs)
        else:
            three = [t[:, None].expand(-1, 3, -1, -1) for t in (q, k, v)]
            fused.kv_append_chunk(*three, p - 2, cos, sin, gq, gk, dc.APPEND_EPS, kc, vc, None, ks, vs)
        got.append([t[:, pos].clone() for t in (kc, ks, vc, vs)])
    for other, writer in zip(got[1:], ("step", "chunk")):
        for a, b, what in zip(got[0], other, ("k codes", "k scales", "v codes", "v scales")):
            nm.assert_bits(b, a, f"{mode}: {what} of the {writer} against the prefill")


# ------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("T", k8.CHUNKS)
@pytest.mark.parametrize("H,Hkv", k8.HEADS)
@pytest.mark.parametrize("D", k8.DIMS)
def test_cached_attention_fp8(D, H, Hkv, T, cuda, monkeypatch):
    hip.require()
    kernels_only(monkeypatch)
    worst = 0.0
    for lens in k8.length_sets(Hkv, T):
        for n_new in (None, k8.ragged(T)):
            worst = max(worst, k8.check_attention_case(fused.cached_attention_fp8, cuda, D, H, Hkv, T, lens, n_new))
    print(f"[kv8] attention D={D} H={H}/{Hkv} T={T}: worst row ratio {worst:.3f} of C_ROWS = {nm.C_ROWS}")


@pytest.mark.parametrize("T", (1, 5))
@pytest.mark.parametrize("H,Hkv", [(8, 2), (7, 1)])
@pytest.mark.parametrize("D", k8.DIMS)
def test_cached_attention_fp8_windows_and_bounds(D, H, Hkv, T, cuda, monkeypatch):
    hip.require()
    kernels_only(monkeypatch)
    worst = 0.0
    for window, lens in k8.WINDOW_CASES:
        worst = max(worst, k8.check_attention_case(fused.cached_attention_fp8, cuda, D, H, Hkv, T, lens, k8.ragged(T), window))
    if T == 5:
        for lens, max_len in k8.BOUND_CASES:
            worst = max(worst, k8.check_attention_case(fused.cached_attention_fp8, cuda, D, H, Hkv, T, lens, None, 0,
                                                       max_len=max_len))
    print(f"[kv8] attention windows / bounds D={D} H={H}/{Hkv} T={T}: worst row ratio {worst:.3f}")


# ------------------------------------------------------------------------------------------- models
def teacher_forced(m, seq, lens, kv_dtype):
    """Logits [B, SEQ, V] (NaN where not computed) of a cached run and its cache: a prefill of max(LENS) columns, one
    single-token step, then chunks of CHUNK tokens per row, ragged where a row runs out of tokens."""
    B, dev = seq.shape[0], seq.device
    W = max(LENS)
    steps = -(-(SEQ - min(LENS) - 1) // CHUNK)
    rows = torch.arange(B, device=dev)
    cache = KVCache(m.config, B, W + 1 + steps * CHUNK, dev, m.lm_head.weight.dtype, kv_dtype)
    out = torch.full((B, SEQ, m.config.vocab_size), float("nan"), device=dev)
    t = torch.arange(CHUNK, device=dev)
    with torch.no_grad():
        prompt = torch.where(torch.arange(W, device=dev)[None] < lens[:, None], seq[:, :W], torch.zeros_like(seq[:, :W]))
        out[rows, lens - 1] = m(prompt, cache=cache).logits[rows, lens - 1].float()
        cache.set_lengths(lens)
        out[rows, lens] = m(seq[rows, lens][:, None], cache=cache).logits[:, 0].float()
        for s in range(steps):
            pos = lens[:, None] + 1 + s * CHUNK + t[None, :]
            live = pos < SEQ
            h = m._decoder()(seq.gather(1, pos.clamp_max(SEQ - 1)), cache=cache, n_new=live.sum(1).to(torch.int32))
            out[rows[:, None].expand_as(pos)[live], pos[live]] = m.lm_head(h).float()[live]
    return out, cache


@pytest.mark.parametrize("family", FAMILIES)
def test_layer0_bits_and_logits(family, cuda, monkeypatch):
    hip.require()
    m, ref = pair(family, cuda)
    seq = torch.randint(1, 256, (3, SEQ), generator=torch.Generator().manual_seed(9)).to(cuda)
    lens = torch.tensor(LENS, device=cuda)
    exact = exact_logits(ref, seq)
    with torch.no_grad():
        full = m(seq).logits.float()
    fused.set_impl("torch")
    try:
        twin8, _ = teacher_forced(ref, seq, lens, "fp8_e4m3")  # the fp32 twin on an fp8 cache: quantisation alone
    finally:
        fused.set_impl("auto")
    plain, cache16 = teacher_forced(m, seq, lens, None)
    kernels_only(monkeypatch)
    got, cache8 = teacher_forced(m, seq, lens, "fp8_e4m3")
    monkeypatch.undo()
    assert cache8.lengths.tolist() == [SEQ] * 3 and cache16.lengths.tolist() == [SEQ] * 3
    for j, what in enumerate(("keys", "values")):
        ec, es = fused.kv_quantize_reference(cache16.layer(0)[j][:, :SEQ])
        nm.assert_bits(cache8.layer(0)[j][:, :SEQ], ec, f"{family}: layer 0 {what}, codes")
        nm.assert_bits(cache8.layer_scales(0)[j][:, :SEQ], es, f"{family}: layer 0 {what}, scales")
    done = ~torch.isnan(got).any(-1)
    assert bool((done == (torch.arange(SEQ, device=cuda)[None] >= (lens - 1)[:, None])).all())
    assert bool(torch.isfinite(got[done]).all())
    err = lambda x: torch.where(done, (torch.nan_to_num(x) - exact).abs().amax(-1), torch.zeros_like(exact[..., 0]))
    e_k, e_q, e_f = err(got), err(twin8), err(full)
    ratio = torch.where(done, e_k / (e_q + e_f), torch.zeros_like(e_k))
    worst = float(ratio.max())
    b, t = (int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape))
    print(f"[kv8] {family}: E_k / (E_q + E_f) max {worst:.3f} at row {b} position {t} (E_k {float(e_k[b, t]):.3e}, E_q "
          f"{float(e_q[b, t]):.3e}, E_f {float(e_f[b, t]):.3e}); median {float(ratio[done].median()):.3f}; E_q / E_f median "
          f"{float((e_q / e_f)[done].median()):.3f}")
    assert worst <= MAX_RATIO
    fused.check_index_errors(blocking=True)


@pytest.mark.parametrize("family", FAMILIES)
def test_generate_fp8(family, cuda, monkeypatch):
    hip.require()
    kernels_only(monkeypatch)
    m, _ = pair(family, cuda)
    a, _ = pair(family, cuda, 101, 1)
    ids = torch.randint(1, 256, (3, 20), generator=torch.Generator().manual_seed(13)).to(cuda)
    mask = torch.ones_like(ids)
    mask[0, :7] = 0
    kw = dict(attention_mask=mask, max_new_tokens=12, kv_cache_dtype="fp8_e4m3")
    out = m.generate(ids, **kw)
    assert out.shape == (3, 32) and torch.equal(out[:, :20], ids)
    assert torch.equal(m.generate(ids, **kw), out)
    eos = int(out[1, 22])  # row 1 stops at its third new token
    stopped = m.generate(ids, eos_token_id=eos, pad_token_id=255, **kw)
    first = int((out[1, 20:] == eos).nonzero()[0])
    assert torch.equal(stopped[1, :21 + first], out[1, :21 + first]) and bool((stopped[1, 21 + first:] == 255).all())
    for extra in (dict(num_beams=3), dict(assistant_model=a)):
        one = m.generate(ids, **kw, **extra)
        assert one.shape[0] == 3 and torch.equal(one[:, :20], ids) and torch.equal(m.generate(ids, **kw, **extra), one)
    fused.check_index_errors(blocking=True)
