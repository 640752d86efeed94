"""kv_append (csrc/decode.hip): the rotated q and the appended k are bit-equal to row pos[b] of fused.rope /
fused.qk_norm_rope, v is copied bit-exact, everything else in the caches keeps its poison pattern, ragged
positions include 0 and Tmax - 1, an out-of-range position raises through check_index_errors and writes nothing
outside the cache, and null tables give a plain append (tests/decode_cases.py)."""
import pytest
import torch

import decode_cases as dc
import numerics as nm
from distributed_lion_pytorch_amd.ops import fused, hip

pytestmark = pytest.mark.gpu


def _kernel_only(monkeypatch):
    monkeypatch.setattr(fused, "kv_append_reference", lambda *a, **kw: pytest.fail("the PyTorch form ran"))


@pytest.mark.parametrize("gains", [False, True])
@pytest.mark.parametrize("D", dc.DIMS)
def test_rotation_and_norm_are_the_training_kernels_bits(D, gains, cuda, monkeypatch):
    hip.require()
    _kernel_only(monkeypatch)
    dc.check_append(fused.kv_append, cuda, D, gains)


@pytest.mark.parametrize("D", dc.DIMS)
def test_null_tables_give_a_plain_append(D, cuda, monkeypatch):
    hip.require()
    _kernel_only(monkeypatch)
    dc.check_append(fused.kv_append, cuda, D, gains=False, tables=False)


@pytest.mark.parametrize("gains", [False, True])
def test_out_of_range_position_raises_and_stays_inside(gains, cuda, monkeypatch):
    hip.require()
    _kernel_only(monkeypatch)
    D, T = 128, dc.APPEND_TMAX
    fused.check_index_errors(blocking=True)  # nothing pending
    qkv, gq, gk, cos, sin = (t.to(cuda) for t in dc.append_inputs(D))
    q, k, v = dc.split_step(qkv, D)
    kc, kbuf = dc.guarded_cache(D, cuda)
    vc, vbuf = dc.guarded_cache(D, cuda)
    pos = torch.tensor([-1, T, T + 100000, 3], dtype=torch.int32, device=cuda)
    fused.kv_append(q, k, v, pos, cos, sin, gq if gains else None, gk if gains else None, dc.APPEND_EPS, kc, vc)
    with pytest.raises(ValueError, match="KV cache"):
        fused.check_index_errors(blocking=True)
    fused.check_index_errors(blocking=True)  # the flag is cleared
    clamped = torch.tensor([0, T - 1, T - 1, 3], device=cuda)
    rows = torch.arange(dc.APPEND_B, device=cuda)
    for cache, buf in ((kc, kbuf), (vc, vbuf)):
        assert bool((buf[:dc.GUARD] == dc.POISON).all()) and bool((buf[-dc.GUARD:] == dc.POISON).all())
        untouched = torch.ones(cache.shape[:2], dtype=torch.bool, device=cuda)
        untouched[rows, clamped] = False
        assert bool((cache[untouched] == dc.POISON).all())
    nm.assert_bits(vc[rows, clamped], v.contiguous(), "v at the clamped positions")


def test_two_runs_are_bit_identical_and_contiguous_inputs_agree(cuda):
    hip.require()
    D = 128
    qkv, gq, gk, cos, sin = (t.to(cuda) for t in dc.append_inputs(D))
    pos = torch.tensor(dc.APPEND_POS, dtype=torch.int32, device=cuda)
    outs = []
    for contiguous in (False, False, True):
        q, k, v = dc.split_step(qkv, D)
        if contiguous:
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        kc, _ = dc.guarded_cache(D, cuda)
        vc, _ = dc.guarded_cache(D, cuda)
        outs.append((fused.kv_append(q, k, v, pos, cos, sin, gq, gk, dc.APPEND_EPS, kc, vc), kc.clone(), vc.clone()))
    for other in outs[1:]:
        for a, b, n in zip(outs[0], other, ("q", "k cache", "v cache")):
            nm.assert_bits(a, b, n)


def test_op_checks(cuda):
    hip.require()
    D = 128
    qkv, gq, gk, cos, sin = (t.to(cuda) for t in dc.append_inputs(D))
    q, k, v = dc.split_step(qkv, D)
    kc, _ = dc.guarded_cache(D, cuda)
    pos = torch.zeros(dc.APPEND_B, dtype=torch.int32, device=cuda)
    flag = fused._index_flag(cuda)
    ops = hip.ops()
    with pytest.raises(RuntimeError, match="pairs"):
        ops.kv_append(q, k, v, pos, cos, None, None, None, 1e-6, kc, kc, flag)
    with pytest.raises(RuntimeError, match="pairs"):
        ops.kv_append(q, k, v, pos, None, None, gq, gk, 1e-6, kc, kc, flag)
    with pytest.raises(RuntimeError, match="cos/sin"):
        ops.kv_append(q, k, v, pos, cos[:5].contiguous(), sin[:5].contiguous(), None, None, 1e-6, kc, kc, flag)
    with pytest.raises(RuntimeError, match="pos"):
        ops.kv_append(q, k, v, pos.long(), cos, sin, None, None, 1e-6, kc, kc, flag)
    with pytest.raises(RuntimeError, match="head_dim"):
        ops.kv_append(q[..., :32], k[..., :32], v[..., :32], pos, None, None, None, None, 1e-6, kc, kc, flag)
