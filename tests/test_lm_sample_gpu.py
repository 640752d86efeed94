"""The LM-head sampling kernel (csrc/lm_sample.hip) and ``fused.lm_head_sample`` on the GPU against the fp64 form
of its contract (tests/lm_sample_cases.py): the floor inside the mass bound, kept and the top-k threshold exact,
the token within delta of the best fp64 Gumbel score; masked and NaN columns, bit-equal repeats, the step in the
hash, the distribution of the draws, and the public op."""
import pytest
import torch

import lm_sample_cases as sc
from distributed_lion_pytorch_amd.ops import fused, hip
from distributed_lion_pytorch_amd.ops.linear import gemm_fwd
from distributed_lion_pytorch_amd.ops.reference import sr_key
from test_lm_sample_cpu import distribution_is_softmax

pytestmark = pytest.mark.gpu

CASES = [(dt, v) for dt in sc.DTYPES for v in sc.VOCABS]


@pytest.mark.parametrize("dtype,v", CASES, ids=[f"{str(d)[6:]}-{v}" for d, v in CASES])
def test_kernel_against_fp64(dtype, v, cuda):
    hip.require()
    for n in (1, 3):
        for setting in sc.SETTINGS:
            x, inv_t, k, p, ref = sc.case(n, v, dtype, setting)
            xd = x.to(cuda)
            out = hip.ops().lm_sample(xd, v, inv_t, k, p, sc.KEY)
            assert [o.dtype for o in out] == [torch.int32, torch.float32, torch.float32, torch.int32]
            assert all(o.shape == (n,) for o in out)
            assert torch.equal(xd.view(torch.uint8).cpu(), x.view(torch.uint8)), "the logits are read-only"
            sc.check(out, x, v, inv_t, k, p, ref, f"{dtype} v={v} N={n} {setting}")
            for a, b in zip(out, hip.ops().lm_sample(xd, v, inv_t, k, p, sc.KEY)):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "same inputs, same bits"


@pytest.mark.parametrize("setting", [(1.0, 0, 1.0), (0.8, 40, 0.95), (1.3, 0, 0.9)])
def test_masked_and_nan_columns(setting, cuda):
    """Row 0: -inf except two columns; row 1: all -inf; row 2: random with NaN columns; over 32 keys."""
    hip.require()
    t, k, p = setting
    v = 4099
    x = sc.rows(3, v, torch.bfloat16, seed=4)
    x[:2, :v] = float("-inf")
    x[0, 7], x[0, 4097] = 1.0, 0.5
    x[2, 100:200] = float("nan")
    x[2, 3000] = float("nan")
    xd = x.to(cuda)
    seen = set()
    for step in range(32):
        ids, lse, floor, kept = hip.ops().lm_sample(xd, v, sc.inv_temperature(t), k, p, sr_key(5, step))
        seen.add(int(ids[0]))
        assert int(ids[1]) == -1 and int(kept[1]) == 0 and float(lse[1]) == float("-inf")
        assert 0 <= int(ids[2]) < v and not bool(torch.isnan(x[2, int(ids[2])])), "a NaN column was drawn"
        assert int(kept[0]) in (1, 2) and float(floor[0]) * t in (pytest.approx(1.0), pytest.approx(0.5))
    assert seen == {7, 4097}


def test_step_changes_the_tokens(cuda):
    hip.require()
    x = sc.rows(64, 513, torch.bfloat16, seed=6).to(cuda)
    a, b = (hip.ops().lm_sample(x, 513, 1.0, 0, 1.0, sr_key(3, step))[0] for step in (0, 1))
    assert not torch.equal(a, b)


def test_distribution(cuda):
    hip.require()
    distribution_is_softmax(lambda x: hip.ops().lm_sample(x.to(cuda), 8, 1.0, 0, 1.0, sc.KEY)[0])


def test_public_op_and_refusals(cuda, monkeypatch):
    hip.require()
    monkeypatch.setattr(fused, "_lm_sample_torch", lambda *a, **kw: pytest.fail("PyTorch lm_sample ran"))
    torch.manual_seed(9)
    h = torch.randn(2, 3, 64, device=cuda).bfloat16()
    w = torch.randn(513, 64, device=cuda).bfloat16()
    with torch.no_grad():
        out = fused.lm_head_sample(h, w, temperature=0.8, top_k=40, top_p=0.95, seed=7, step=2)
    logits = gemm_fwd(h.view(-1, 64), fused._pad_rows(w))
    want = hip.ops().lm_sample(logits, 513, sc.inv_temperature(0.8), 40, 0.95, sr_key(7, 2))
    assert all(torch.equal(a, b) for a, b in zip(out, want)) and out.ids.shape == (6,)
    with pytest.raises(RuntimeError, match="forward-only"):
        fused.lm_head_sample(h.clone().requires_grad_(), w)
    for bad in (dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1)):
        with pytest.raises(RuntimeError, match="lm_sample needs"):
            hip.ops().lm_sample(logits, 513, 1.0, bad.get("top_k", 0), bad.get("top_p", 1.0), 0)
    with pytest.raises(RuntimeError):
        hip.ops().lm_sample(logits[:, :100], 100, 1.0, 0, 1.0, 0)  # not contiguous
    torch.cuda.synchronize()
