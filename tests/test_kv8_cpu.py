"""The fp8 KV cache on the CPU: the quantiser's definition (fused.kv_quantize_reference), the PyTorch forms of the fp8
appends and of cached_attention_fp8, and generate(kv_cache_dtype="fp8_e4m3") on fp32 tiny models.
docs/TEST_TOLERANCES.md "FP8 KV cache"."""
import pytest
import torch

import kv8_cases as k8
from distributed_lion_pytorch_amd.models import KVCache
from distributed_lion_pytorch_amd.ops import fused
from test_speculative_gpu import FAMILIES, build

CPU = torch.device("cpu")


def _check_definition(x, name):
    codes, scale = fused.kv_quantize_reference(x)
    xf = x.float()
    a = xf.abs().amax(-1)
    assert codes.dtype == torch.uint8 and scale.dtype == torch.float32
    assert bool((torch.frexp(scale).mantissa == 0.5).all()), name + ": a scale that is no power of two"
    free = a >= 2.0 ** -118  # e is not clamped
    r = a[free].double() / scale[free].double()
    assert bool(((r >= 224) & (r < 448)).all()), name + ": absmax / scale outside [224, 448)"
    deq = fused.kv_dequantize(codes, scale)
    bound = torch.maximum(2.0 ** -4 * xf.abs(), 2.0 ** -10 * scale[..., None])
    assert bool(((deq - xf).abs() <= bound).all()), name + ": dequantisation error"
    return codes, scale, deq


def test_quantiser_definition_random():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(64, 3, 128, generator=g) * torch.exp2(torch.randint(-30, 30, (64, 3, 1), generator=g))).to(torch.bfloat16)
    _check_definition(x, "random")


def test_quantiser_hand_rows():
    rows = k8.hand_rows()
    got = {n: _check_definition(r[None], n) for n, r in rows.items()}
    c, s, d = got["zeros"]
    assert bool((c == 0).all()) and float(s) == 2.0 ** -126
    assert float(got["absmax 1.75"][1]) == 2.0 ** -7 and int(got["absmax 1.75"][0][0, 0]) == 0x76  # 224
    assert float(got["absmax below 1.75"][1]) == 2.0 ** -8 and int(got["absmax below 1.75"][0][0, 0]) == 0x7E  # 446 -> 448
    c, s, _ = got["subnormal codes and ties"]
    assert float(s) == 2.0 ** -8 and c[0, :7].tolist() == [0x78, 0x01, 0x00, 0x02, 0x80, 0x38, 0x3A]
    assert got["negative zero"][0][0, :2].tolist() == [0x78, 0x80]
    c, s, _ = got["absmax 2^-120"]
    assert float(s) == 2.0 ** -126 and c[0, :3].tolist() == [0x68, 0xC8, 0x18]  # 64, -4, 1 / 16
    assert float(got["absmax 2^-117"][1]) == 2.0 ** -125 and got["absmax 2^-117"][0][0, :2].tolist() == [0x78, 0x30]
    c, s, _ = got["absmax 2^120"]
    assert float(s) == 2.0 ** 112 and c[0, :3].tolist() == [0xF8, 0x38, 0x00]


@pytest.mark.parametrize("T", [1, 5])
def test_attention_pytorch_form(T):
    for lens in k8.length_sets(1, T)[::2]:
        k8.check_attention_case(fused.cached_attention_fp8, CPU, 64, 8, 1, T, lens, k8.ragged(T), splits=(None,))
    k8.check_attention_case(fused.cached_attention_fp8, CPU, 64, 4, 4, T, (0, 65, 300), None, window=16, splits=(None,))


@pytest.mark.parametrize("family", FAMILIES)
def test_speculative_equals_greedy_on_an_fp8_cache(family):
    m, a = build(family), build(family, seed=7, layers=1)
    ids = torch.randint(1, 256, (3, 12), generator=torch.Generator().manual_seed(3))
    mask = torch.ones_like(ids)
    mask[0, :5] = 0
    plain = m.generate(ids, attention_mask=mask, max_new_tokens=14, kv_cache_dtype="fp8_e4m3")
    assert plain.shape == (3, 26) and torch.equal(plain[:, :12], ids)
    spec = m.generate(ids, attention_mask=mask, max_new_tokens=14, kv_cache_dtype="fp8_e4m3", assistant_model=a)
    assert torch.equal(spec, plain)


def test_reorder_rows_moves_the_scales(monkeypatch):
    """Beam search on an fp8 cache equals itself with reorder_rows replaced by a move of codes and scales written out
    by hand; moving the codes alone gives other tokens (the rows' scales differ)."""
    m = build("llama")
    ids = torch.randint(1, 256, (2, 9), generator=torch.Generator().manual_seed(5))
    kw = dict(max_new_tokens=8, num_beams=3, kv_cache_dtype="fp8_e4m3")
    out = m.generate(ids, **kw)

    def by_hand(self, index, lo=0, scales=True):
        for buf in (self._buf, self._scales) if scales else (self._buf,):
            moved = torch.stack([buf[:, :, int(i)] for i in index], dim=2)
            buf[:, :, :, lo:self.width] = moved[:, :, :, lo:self.width]
        self.lengths.copy_(self.lengths[index])

    monkeypatch.setattr(KVCache, "reorder_rows", by_hand)
    assert torch.equal(m.generate(ids, **kw), out)
    monkeypatch.setattr(KVCache, "reorder_rows", lambda self, index, lo=0: by_hand(self, index, lo, scales=False))
    assert not torch.equal(m.generate(ids, **kw), out)


def test_errors():
    m = build("gpt2")
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        m.generate(torch.ones(1, 4, dtype=torch.long), max_new_tokens=2, kv_cache_dtype="int8")
    with pytest.raises(ValueError, match="kv_dtype"):
        KVCache(m.config, 1, 8, kv_dtype="fp8")
