"""The PyTorch form of the LM-head top-k (fused._lm_topk_torch) against the oracle of
tests/lm_topk_cases.py on the case and tie generators of the GPU test: the
reference alone meets every condition tests/test_lm_topk_gpu.py sets; and
fused.lm_head_topk on the CPU."""
import pytest
import torch

import numerics as nm
from distributed_lion_pytorch_amd.ops import fused
from lm_topk_cases import check_tie_rows, padded, random_rows, reference_topk, tie_rows_topk

CPU = torch.device("cpu")
CASES = [(dt, V) for dt in (torch.bfloat16, torch.float16) for V in (100, 512, 4104, 50257)] + \
        [(torch.float32, 100), (torch.float32, 50257)]


def _check(x, V, k, name, ref):
    values, ids, lse = fused._lm_topk_torch(x, V, k)
    assert values.dtype == lse.dtype == torch.float32 and ids.dtype == torch.int32
    assert torch.equal(ids.long(), ref[1][:, :k]) and bool((values == ref[0][:, :k]).all()), name
    nm.assert_elems_close(lse, ref[2], 1e-5, 1e-5, f"{name} lse")
    return values, ids


@pytest.mark.parametrize("dtype,V", CASES, ids=[f"{str(dt).split('.')[1]}-{V}" for dt, V in CASES])
def test_torch_form_against_the_oracle(dtype, V):
    x = random_rows(12, V, dtype, CPU, seed=12)
    ref = reference_topk(x, V, 64)
    for k in (1, 2, 8, 64):
        _check(x, V, k, f"{dtype} V={V} k={k}", ref)
    if V == 100:
        x = random_rows(12, 64, dtype, CPU, seed=3)
        _check(x, 64, 64, f"{dtype} k = v", reference_topk(x, 64, 64))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bfloat16", "float32"])
def test_torch_form_on_tie_rows(dtype):
    V = 50257
    x, first = tie_rows_topk(V, padded(V), dtype, CPU)
    ref = reference_topk(x, V, 64)
    for k in (1, 2, 8, 21, 41, 64):
        values, ids = _check(x, V, k, f"ties {dtype} k={k}", ref)
        check_tie_rows(values, ids, x, V, k, first)


def test_lm_head_topk_on_the_cpu():
    torch.manual_seed(0)
    h, w = torch.randn(3, 4, 32), torch.randn(97, 32)
    with pytest.raises(RuntimeError, match="forward-only"):
        fused.lm_head_topk(h, w.clone().requires_grad_(), 5)
    for bad in (0, 98):
        with pytest.raises(ValueError, match="k"):
            fused.lm_head_topk(h, w, bad)
    with torch.no_grad():
        out = fused.lm_head_topk(h, w, 5)
    logits = h.view(-1, 32) @ w.t()
    ref_values, ref_ids, ref_lse = reference_topk(logits, 97, 5)
    assert out.values.shape == out.ids.shape == (12, 5) and out.lse.shape == (12,)
    assert torch.equal(out.ids.long(), ref_ids) and out.ids.dtype == torch.int32
    nm.assert_elems_close(out.values, ref_values.double(), 1e-5, 1e-5, "cpu values")
    nm.assert_elems_close(out.lse, ref_lse, 1e-5, 1e-5, "cpu lse")
    # the log-probabilities a beam step adds: values - lse
    logp = torch.log_softmax(logits.double(), -1).gather(1, ref_ids)
    nm.assert_elems_close(out.values - out.lse[:, None], logp, 1e-5, 1e-5, "cpu log-probabilities")
