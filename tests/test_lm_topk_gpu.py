"""The LM-head top-k kernel (csrc/lm_topk.hip) and ``fused.lm_head_topk`` on the GPU:
ids and values exactly equal to the stable-sort oracle (tests/lm_topk_cases.py) on
random, tie and non-finite rows, the logsumexp under the scoring kernel's bound,
the binding's refusals, and the op on exact integer operands."""
import pytest
import torch

import numerics as nm
from distributed_lion_pytorch_amd.ops import fused, hip
from lm_topk_cases import check_tie_rows, padded, random_rows, reference_topk, tie_rows_topk

pytestmark = pytest.mark.gpu

VOCABS = (100, 512, 4104, 50257, 128256)  # 4104: one chunk past a full 512-thread iteration
CASES = [(dt, V) for dt in (torch.bfloat16, torch.float16) for V in VOCABS] + \
        [(torch.float32, 100), (torch.float32, 50257)]
KS = (1, 2, 8, 64)


def _ids(cases):
    return [f"{str(dt).split('.')[1]}-{V}" for dt, V in cases]


def _check(x, V, k, name, rows=slice(None), ref=None):
    """ref: reference_topk(x, V, k') for some k' >= k, computed once per x."""
    keep = x.clone()
    values, ids, lse = hip.ops().lm_topk(x, V, k)
    assert values.dtype == lse.dtype == torch.float32 and ids.dtype == torch.int32
    assert values.shape == ids.shape == (x.shape[0], k) and lse.shape == (x.shape[0],)
    assert torch.equal(x.view(torch.uint8), keep.view(torch.uint8)), "the logits are read-only"
    ref_values, ref_ids, ref_lse = ref if ref is not None else reference_topk(x, V, k)
    ref_values, ref_ids = ref_values[:, :k], ref_ids[:, :k]
    assert torch.equal(ids.long()[rows], ref_ids[rows]), f"{name} ids"
    assert bool((values[rows] == ref_values[rows]).all()), f"{name} values"
    nm.assert_elems_close(lse[rows], ref_lse[rows], 1e-5, 1e-5, f"{name} lse")
    again = hip.ops().lm_topk(x, V, k)
    for a, b in zip((values, ids, lse), again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{name}: same inputs, same bits"
    return values, ids, lse


@pytest.mark.parametrize("dtype,V", CASES, ids=_ids(CASES))
def test_kernel_against_the_stable_sort(dtype, V, cuda):
    hip.require()
    for N in (1, 12):
        x = random_rows(N, V, dtype, cuda, seed=N)
        ref = reference_topk(x, V, 64)
        for k in KS:
            _check(x, V, k, f"{dtype} V={V} N={N} k={k}", ref=ref)
        if dtype == torch.bfloat16 and V == 128256 and N == 12:
            top = ref[0]
            assert bool((top[:, 1:] == top[:, :-1]).any()), "bf16 rows of this width tie inside the top 64"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bfloat16", "float16", "float32"])
def test_k_equal_to_the_vocabulary(dtype, cuda):
    hip.require()
    x = random_rows(12, 64, dtype, cuda, seed=3)
    _, ids, _ = _check(x, 64, 64, f"{dtype} k = v = 64")
    assert torch.equal(ids.long().sort(dim=1).values, torch.arange(64, device=cuda).expand(12, 64))


TIE_CASES = [(dt, V) for dt in (torch.bfloat16, torch.float32) for V in (50257, 128256)]


@pytest.mark.parametrize("dtype,V", TIE_CASES, ids=_ids(TIE_CASES))
def test_tie_rows(dtype, V, cuda):
    hip.require()
    x, first = tie_rows_topk(V, padded(V), dtype, cuda)
    ref = reference_topk(x, V, 64)
    for k in KS + (21, 41):
        values, ids, _ = _check(x, V, k, f"ties {dtype} V={V} k={k}", ref=ref)
        check_tie_rows(values, ids, x, V, k, first)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bfloat16", "float32"])
def test_non_finite_rows(dtype, cuda):
    """A -inf block (masked vocabulary) is ordinary input.  NaN and +inf are
    tolerated: the ids stay distinct columns of the row and the other rows of the
    launch are unaffected."""
    hip.require()
    torch.manual_seed(5)
    V, Vp, N = 50257, 50304, 12
    x = (2 * torch.randn(N, Vp, device=cuda)).to(dtype)
    x[:, V:] = 1e4
    x[0, 1000:20000] = float("-inf")
    x[1, :40000] = float("-inf")  # whole threads see nothing finite
    x[6, 10:] = float("-inf")  # fewer than k finite columns: the lowest -inf columns fill the rest
    x[2, 5] = float("nan")
    x[3, 7] = float("inf")
    x[4] = float("nan")
    x[5] = float("-inf")
    bad = [2, 3, 4, 5]
    good = [i for i in range(N) if i not in bad]
    ref = reference_topk(x, V, 64)
    for k in (8, 64):
        _, ids, _ = _check(x, V, k, f"non-finite {dtype} k={k}", rows=good, ref=ref)
        assert bool(((ids >= 0) & (ids < V)).all()), ids.tolist()
        srt = ids.long().sort(dim=1).values
        assert bool((srt[:, 1:] != srt[:, :-1]).all()), "ids are distinct within a row"
        assert ids[6, 10:].tolist() == list(range(10, k))
    torch.cuda.synchronize()


def test_refusals(cuda):
    hip.require()
    x = random_rows(2, 100, torch.bfloat16, cuda)
    for k in (0, 65):
        with pytest.raises(RuntimeError, match="1 <= k <= 64"):
            hip.ops().lm_topk(x, 100, k)
    with pytest.raises(RuntimeError, match="k <= v"):
        hip.ops().lm_topk(x, 40, 41)
    flat = torch.zeros(2 * 128 + 8, device=cuda, dtype=torch.bfloat16)
    off = flat[1:1 + 2 * 128].view(2, 128)  # contiguous, 2 bytes off a 16-byte boundary
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    with pytest.raises(RuntimeError):
        hip.ops().lm_topk(off, 100, 4)
    torch.cuda.synchronize()


def test_op_on_exact_integer_operands(cuda, monkeypatch):
    """h and W hold integers in [-2, 2]: |h . w| <= 256 is exact in bf16 whatever
    GEMM runs, ties are everywhere, and ids / values have one right answer."""
    hip.require()
    monkeypatch.setattr(fused, "_lm_topk_torch", lambda *a, **kw: pytest.fail("PyTorch lm_topk ran"))
    torch.manual_seed(7)
    V, C, k = 50257, 64, 16
    h = torch.randint(-2, 3, (2, 6, C), device=cuda).bfloat16()
    w = torch.randint(-2, 3, (V, C), device=cuda).bfloat16()
    logits = h.double().view(-1, C) @ w.double().t()
    assert logits.abs().max().item() <= 256
    with torch.no_grad():
        out = fused.lm_head_topk(h, w, k)
    ref_values, ref_ids, ref_lse = reference_topk(logits, V, k)
    assert out.ids.dtype == torch.int32 and out.ids.shape == (12, k)
    assert torch.equal(out.ids.long(), ref_ids) and bool((out.values == ref_values).all())
    assert bool((ref_values[:, 1:] == ref_values[:, :-1]).any()), "the case is meant to have ties inside the top k"
    nm.assert_elems_close(out.lse, ref_lse, 1e-5, 1e-5, "op lse")
    with pytest.raises(RuntimeError, match="forward-only"):
        fused.lm_head_topk(h.clone().requires_grad_(), w, k)
    with pytest.raises(ValueError, match="k"):
        fused.lm_head_topk(h, w, 0)
