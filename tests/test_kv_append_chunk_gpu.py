"""fused.kv_append_chunk on the GPU (csrc/chunk_attention.hip): bit-equal to fused.rope / fused.qk_norm_rope at the
tokens' positions, writes exactly the live tokens' cache rows (guarded caches, tests/chunk_cases.py), and a chunk
that runs past the cache is an error that leaves the guard bands intact."""
import pytest
import torch

import chunk_cases as cc
import decode_cases as dc
from distributed_lion_pytorch_amd.ops import fused, hip

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def kernels_only(monkeypatch):
    hip.require()
    monkeypatch.setattr(fused, "kv_append_chunk_reference", lambda *a, **kw: pytest.fail("PyTorch kv_append_chunk ran"))


@pytest.mark.parametrize("mode", cc.MODES)
@pytest.mark.parametrize("D", cc.DIMS)
@pytest.mark.parametrize("T", [1, 3, 8])
def test_append_chunk(T, D, mode, cuda):
    cc.check_append_chunk(fused.kv_append_chunk, cuda, D, T, mode)
    fused.check_index_errors(blocking=True)


@pytest.mark.parametrize("D", cc.DIMS)
def test_without_n_new_every_token_is_written(D, cuda):
    T = 3
    q, k, v = cc.split_chunk(cc.append_inputs(D, T).to(cuda), D)
    kc, _ = dc.guarded_cache(D, cuda)
    vc, _ = dc.guarded_cache(D, cuda)
    pos = torch.tensor((0, 4, 9, dc.APPEND_TMAX - T), dtype=torch.int32, device=cuda)
    q_out = fused.kv_append_chunk(q, k, v, pos, None, None, None, None, 0.0, kc, vc)
    assert torch.equal(q_out, q)
    for b in range(dc.APPEND_B):
        p = int(pos[b])
        assert torch.equal(kc[b, p:p + T], k[b]) and torch.equal(vc[b, p:p + T], v[b])
    assert int((kc == dc.POISON).all(-1).all(-1).sum()) == dc.APPEND_B * (dc.APPEND_TMAX - T)
    fused.check_index_errors(blocking=True)


@pytest.mark.parametrize("mode", ["append", "norm_rope"])
def test_chunk_past_the_cache_is_an_error(mode, cuda):
    D, T = 64, 3
    _, gq, gk, cos, sin = (t.to(cuda) for t in dc.append_inputs(D))
    if mode == "append":
        gq = gk = cos = sin = None
    q, k, v = cc.split_chunk(cc.append_inputs(D, T).to(cuda), D)
    kc, kbuf = dc.guarded_cache(D, cuda)
    vc, vbuf = dc.guarded_cache(D, cuda)
    fused.check_index_errors(blocking=True)
    # row 1's last token would land at TMAX; row 2 starts below 0; row 3's overrun is not live (n_new) and is no error
    pos = torch.tensor((0, dc.APPEND_TMAX - T + 1, -1, dc.APPEND_TMAX - 1), dtype=torch.int32, device=cuda)
    n_new = torch.tensor((T, T, T, 1), dtype=torch.int32, device=cuda)
    fused.kv_append_chunk(q, k, v, pos, cos, sin, gq, gk, dc.APPEND_EPS, kc, vc, n_new)
    with pytest.raises(ValueError, match="KV cache"):
        fused.check_index_errors(blocking=True)
    for buf in (kbuf, vbuf):
        assert bool((buf[:dc.GUARD] == dc.POISON).all()) and bool((buf[-dc.GUARD:] == dc.POISON).all())
    fused.check_index_errors(blocking=True)  # the flag was cleared
    # the same call with row 3 alone: a dead overrun raises nothing
    kc2, _ = dc.guarded_cache(D, cuda)
    vc2, _ = dc.guarded_cache(D, cuda)
    pos = torch.tensor((0, 0, 0, dc.APPEND_TMAX - 1), dtype=torch.int32, device=cuda)
    fused.kv_append_chunk(q, k, v, pos, cos, sin, gq, gk, dc.APPEND_EPS, kc2, vc2, n_new)
    fused.check_index_errors(blocking=True)
