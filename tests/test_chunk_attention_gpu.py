"""fused.chunk_attention on the GPU (csrc/chunk_attention.hip): T queries per sequence against the cache, judged
row by row on numerics.attention_ref64 and its rounding model at the project's C_ROWS -- the criterion
decode_attention is held to (tests/chunk_cases.py; docs/TEST_TOLERANCES.md "Chunk attention / speculative
decoding" has the measured ratios).  Chunk sizes and base lengths around 64 and the split boundaries, ragged
n_new, windows, forced split counts, a shared k|v buffer, NaN beyond the lengths, repeatability, and T = 1 on the
decode cases."""
import pytest
import torch

import chunk_cases as cc
import decode_cases as dc
import numerics as nm
from distributed_lion_pytorch_amd.ops import fused, hip

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def kernels_only(monkeypatch):
    hip.require()
    monkeypatch.setattr(fused, "chunk_attention_reference", lambda *a, **kw: pytest.fail("PyTorch chunk_attention ran"))
    monkeypatch.setattr(fused, "decode_attention_reference", lambda *a, **kw: pytest.fail("PyTorch decode_attention ran"))


@pytest.mark.parametrize("D", cc.DIMS)
@pytest.mark.parametrize("H,Hkv", cc.HEADS)
def test_chunk_sizes_and_lengths(D, H, Hkv, cuda):
    worst = 0.0
    for T in cc.CHUNKS:
        for lens in cc.length_sets(Hkv, T):
            worst = max(worst, cc.check_attention_case(fused.chunk_attention, cuda, D, H, Hkv, T, lens, splits=(None,)))
    print(f"[chunk] D={D} H={H}/{Hkv}: worst ratio over chunk sizes and lengths {worst:.3f}")


@pytest.mark.parametrize("D", cc.DIMS)
@pytest.mark.parametrize("H,Hkv", [(8, 2), (8, 1)])
def test_forced_splits(D, H, Hkv, cuda):
    worst = 0.0
    for T in (2, 8):
        lens = cc.length_sets(Hkv, T)[1]
        worst = max(worst, cc.check_attention_case(fused.chunk_attention, cuda, D, H, Hkv, T, lens))
    print(f"[chunk] D={D} H={H}/{Hkv}: worst ratio over forced splits {worst:.3f}")


@pytest.mark.parametrize("D", cc.DIMS)
@pytest.mark.parametrize("H,Hkv", cc.HEADS)
def test_ragged_n_new(D, H, Hkv, cuda):
    for T in (2, 5, 8):
        for lens in cc.length_sets(Hkv, T):
            cc.check_attention_case(fused.chunk_attention, cuda, D, H, Hkv, T, lens, n_new=cc.ragged(T), splits=(None, 2))


@pytest.mark.parametrize("D", cc.DIMS)
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 1)])
def test_windows(D, H, Hkv, cuda):
    for window, lens in cc.WINDOW_CASES:
        for T in (1, 5, 8):
            cc.check_attention_case(fused.chunk_attention, cuda, D, H, Hkv, T, lens, window=window,
                                    splits=(None, 2, fused._DECODE_MAX_SPLITS))
        cc.check_attention_case(fused.chunk_attention, cuda, D, H, Hkv, 5, lens, n_new=cc.ragged(5), window=window,
                                splits=(None,))


@pytest.mark.parametrize("D", cc.DIMS)
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2)])
def test_host_bound(D, H, Hkv, cuda):
    """max_len below Tmax, as the models pass it (cache.width + T): it sizes the grid, and a row beyond it is clamped."""
    for lens, max_len in cc.BOUND_CASES:
        cc.check_attention_case(fused.chunk_attention, cuda, D, H, Hkv, 5, lens, max_len=max_len)
    lens, max_len = cc.BOUND_CASES[0]
    cc.check_attention_case(fused.chunk_attention, cuda, D, H, Hkv, 5, lens, n_new=cc.ragged(5), window=16, max_len=max_len,
                            splits=(None, 2))


@pytest.mark.parametrize("D", cc.DIMS)
def test_shared_cache(D, cuda):
    cc.check_attention_case(fused.chunk_attention, cuda, D, 8, 2, 5, cc.length_sets(2, 5)[0], shared_cache=True)


@pytest.mark.parametrize("D", cc.DIMS)
@pytest.mark.parametrize("H,Hkv", cc.HEADS)
def test_one_token_is_decode_attention(D, H, Hkv, cuda):
    """T = 1 on decode_cases' inputs (kv_len there counts the query's own key: the chunk form takes kv_len - 1 and
    n_new = 0 for a row without keys), against the same reference and bound."""
    for lens in dc.length_sets(Hkv):
        c = dc.attention_case(D, H, Hkv, tuple(lens))
        q = c["qkv"].to(cuda)[:, :H * D].view(dc.B, 1, H, D)
        k, v = c["k"].to(cuda), c["v"].to(cuda)
        kv_len = c["kv_len"].to(cuda)
        n_new = (kv_len > 0).to(torch.int32)
        for s in dc.FORCED_SPLITS:
            out = fused.chunk_attention(q, k, v, kv_len - n_new, n_new, 0, None, splits=s)
            name = f"chunk T=1 D={D} H={H}/{Hkv} lens={tuple(lens)} splits={s}"
            nm.assert_rows_close(out[:, 0].cpu(), c["ref"], c["model"], nm.C_ROWS, name=name)
            assert bool((out[kv_len == 0] == 0).all()), name + ": a row without keys must be zero"
