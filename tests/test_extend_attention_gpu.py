"""fused.extend_attention (csrc/extend_attention.hip) and fused.kv_append_chunk above 8 tokens per row, through the
cases, fp64 references and checks of tests/chunk_cases.py: the row-wise bound at numerics.C_ROWS, NaN beyond every
length, zero rows past n_new, a second run with the same bits.  T sits on either side of the kernel's token tile."""
import pytest
import torch

import chunk_cases as cc
from distributed_lion_pytorch_amd.ops import fused, hip

pytestmark = pytest.mark.gpu

TQ = fused.EXTEND_TQ
TOKENS = sorted({9, 16, 17, TQ - 1, TQ + 1, 2 * TQ + 1})
SPLITS = (None, 1, 2, fused._EXTEND_MAX_SPLITS)


def length_sets(Hkv, T):
    """Base lengths: an empty cache (causal self-attention), len + T on 63 / 64 / 65, on either side of the first
    split boundary of the unforced grid, and a row that ends exactly at TMAX."""
    splits, c = fused.extend_splits(cc.B, Hkv, cc.TMAX, T)
    assert splits >= 2, "the cases are meant to cross a split boundary of the unforced grid"
    return [(0, 0, 0), (63 - T, 64 - T, 65 - T), (c - 1 - T, c - T, c + 1 - T), (cc.TMAX - T, 2 * c - T, 1)]


def kernel_only(monkeypatch):
    for name in ("extend_attention_reference", "chunk_attention_reference", "kv_append_chunk_reference"):
        monkeypatch.setattr(fused, name, lambda *a, _n=name, **kw: pytest.fail(f"PyTorch {_n} ran"))


@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("H,Hkv", cc.HEADS)
@pytest.mark.parametrize("D", cc.DIMS)
def test_lengths_and_splits(D, H, Hkv, T, cuda, monkeypatch):
    hip.require()
    kernel_only(monkeypatch)
    for lens in length_sets(Hkv, T):
        cc.check_attention_case(fused.extend_attention, cuda, D, H, Hkv, T, lens, splits=SPLITS)


@pytest.mark.parametrize("T", (9, TQ + 1, 2 * TQ + 1))
@pytest.mark.parametrize("H,Hkv", cc.HEADS)
@pytest.mark.parametrize("D", cc.DIMS)
def test_ragged_windows_bounds_and_a_shared_buffer(D, H, Hkv, T, cuda, monkeypatch):
    hip.require()
    kernel_only(monkeypatch)
    fn = fused.extend_attention
    cc.check_attention_case(fn, cuda, D, H, Hkv, T, length_sets(Hkv, T)[2], n_new=cc.ragged(T), splits=SPLITS)
    for window, lens in cc.WINDOW_CASES:
        cc.check_attention_case(fn, cuda, D, H, Hkv, T, lens, window=window, splits=SPLITS)
    cc.check_attention_case(fn, cuda, D, H, Hkv, T, cc.WINDOW_CASES[1][1], n_new=cc.ragged(T), window=16, splits=SPLITS,
                            shared_cache=True)
    for lens, max_len in cc.BOUND_CASES:  # a host bound just above the longest row, and one that a row exceeds
        cc.check_attention_case(fn, cuda, D, H, Hkv, T, lens, max_len=max_len, splits=SPLITS)


@pytest.mark.parametrize("mode", cc.MODES)
@pytest.mark.parametrize("T", (9, 17, 26))
@pytest.mark.parametrize("D", cc.DIMS)
def test_kv_append_chunk_above_8_tokens(D, T, mode, cuda, monkeypatch):
    hip.require()
    kernel_only(monkeypatch)
    cc.check_append_chunk(fused.kv_append_chunk, cuda, D, T, mode)
    fused.check_index_errors(blocking=True)
