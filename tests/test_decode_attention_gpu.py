"""The decode-attention kernel (csrc/decode.hip) against the last query row of numerics.attention_ref64, row by
row at the existing C_ROWS (tests/decode_cases.py): head_dim 64 / 128, group sizes 1, 4, 7 and 8, ragged lengths
around 64, around the kernel's own split boundaries and up to Tmax, windows, a host bound below Tmax, q as a
strided view of the packed q|k|v rows, NaN beyond every row's length, forced split counts 1 / 2 / the maximum,
and bit-identical repeats."""
import pytest
import torch

import decode_cases as dc
from distributed_lion_pytorch_amd.ops import fused, hip

pytestmark = pytest.mark.gpu


def _kernel_only(monkeypatch):
    monkeypatch.setattr(fused, "decode_attention_reference", lambda *a, **kw: pytest.fail("the PyTorch form ran"))


@pytest.mark.parametrize("H,Hkv", dc.HEADS)
@pytest.mark.parametrize("D", dc.DIMS)
def test_lengths_and_splits(D, H, Hkv, cuda, monkeypatch):
    hip.require()
    _kernel_only(monkeypatch)
    for lens in dc.length_sets(Hkv):
        dc.check_attention_case(fused.decode_attention, cuda, D, H, Hkv, lens)


@pytest.mark.parametrize("window,lens", dc.WINDOW_CASES)
@pytest.mark.parametrize("D", dc.DIMS)
def test_windows(D, window, lens, cuda, monkeypatch):
    hip.require()
    _kernel_only(monkeypatch)
    dc.check_attention_case(fused.decode_attention, cuda, D, 8, 2, lens, window=window)


@pytest.mark.parametrize("D", dc.DIMS)
def test_host_bound_below_tmax_and_shared_buffer(D, cuda, monkeypatch):
    """max_len = 200 under Tmax = 520: the grid is sized by max_len, a kv_len above it is clamped to it (the cache
    is NaN from there on), and k / v may be the two halves of one buffer."""
    hip.require()
    _kernel_only(monkeypatch)
    dc.check_attention_case(fused.decode_attention, cuda, D, 8, 2, (200, 250, 77), max_len=200)
    dc.check_attention_case(fused.decode_attention, cuda, D, 4, 4, (200, 1, 199), window=16, max_len=200,
                            shared_cache=True)


def test_split_rule_uses_host_values_only():
    """More rows or kv heads: fewer splits; a window bounds the span; the count never exceeds the maximum and
    every key has a split."""
    for B, Hkv, max_len, window in [(1, 8, 8192, 0), (8, 8, 8192, 0), (32, 8, 2048, 0), (8, 12, 1024, 0),
                                    (1, 1, 100000, 0), (1, 8, 8192, 4096), (3, 1, 520, 0), (2, 2, 1, 0)]:
        s, chunk = fused.decode_splits(B, Hkv, max_len, window)
        span = window if 0 < window < max_len else max_len
        assert 1 <= s <= fused._DECODE_MAX_SPLITS and s * chunk >= span and (s - 1) * chunk < span, (B, Hkv, max_len)
    assert fused.decode_splits(1, 8, 8192)[0] > fused.decode_splits(32, 8, 8192)[0]


def test_op_checks(cuda):
    hip.require()
    q = torch.zeros(2, 4, 128, dtype=torch.bfloat16, device=cuda)
    kc = torch.zeros(2, 16, 2, 128, dtype=torch.bfloat16, device=cuda)
    n = torch.ones(2, dtype=torch.int32, device=cuda)
    ops = hip.ops()
    with pytest.raises(RuntimeError, match="splits"):
        ops.decode_attention(q, kc, kc, n, 0, 16, 0, 16)
    with pytest.raises(RuntimeError, match="failed"):
        ops.decode_attention(q, kc, kc, n, 0, 16, 2, 4)  # 2 x 4 keys do not cover 16
    with pytest.raises(RuntimeError, match="kv_len"):
        ops.decode_attention(q, kc, kc, n.long(), 0, 16, 1, 16)
    with pytest.raises(RuntimeError, match=r"H / Hkv"):
        ops.decode_attention(q[:, :3], kc, kc, n, 0, 16, 1, 16)
    with pytest.raises(RuntimeError, match="token-major"):
        ops.decode_attention(q, kc.transpose(1, 2).contiguous().transpose(1, 2), kc, n, 0, 16, 1, 16)
