"""The LM-head scoring kernel (csrc/lm_score.hip) and everything above it on the
GPU: the kernel against fp64 (loss, logsumexp) and against exact integer
functions of the stored logits (top-1 token, label rank) on edge, tie and
non-finite rows; the op on exact integer operands; ``predictions=True`` on the
native models against their default evaluation path."""
import pytest
import torch
import transformers

import numerics as nm
from distributed_lion_pytorch_amd.models import llama as L
from distributed_lion_pytorch_amd.models.gpt2 import GPT2LMHeadModel, gpt2_config
from distributed_lion_pytorch_amd.ops import fused, hip
from lm_score_cases import reference_score, tie_rows
from test_xent_options_gpu import _edge_rows

pytestmark = pytest.mark.gpu

OPTIONS = [(0.0, 0.0), (0.1, 0.0), (0.1, 1e-3)]
CASES = [(dt, V) for dt in (torch.bfloat16, torch.float16) for V in (100, 512, 32000, 50257, 128256)] + \
        [(torch.float32, 100), (torch.float32, 50257)]
THREADS = 512  # kScoreThreads: 8 columns per thread and iteration


def _ids(cases):
    return [f"{str(dt).split('.')[1]}-{V}" for dt, V in cases]


def _check(x, labels, V, eps, zeta, name, rows=slice(None)):
    keep = x.clone()
    loss, lse, pred, rank = hip.ops().lm_score(x, labels, V, eps, zeta)
    assert loss.dtype == lse.dtype == torch.float32 and pred.dtype == rank.dtype == torch.int32
    assert torch.equal(x.view(torch.uint8), keep.view(torch.uint8)), "the logits are read-only"
    ref_loss, ref_lse, ref_pred, ref_rank = reference_score(x, labels, V, eps, zeta)
    nm.assert_elems_close(loss[rows], ref_loss[rows], 1e-5, 1e-5, f"{name} loss")
    nm.assert_elems_close(lse[rows], ref_lse[rows], 1e-5, 1e-5, f"{name} lse")
    assert torch.equal(pred.long()[rows], ref_pred[rows]), f"{name} pred"
    assert torch.equal(rank.long()[rows], ref_rank[rows]), f"{name} rank"
    ignored = ((labels < 0) | (labels >= V))[rows]
    assert loss[rows][ignored].abs().sum().item() == 0.0 and bool((rank[rows][ignored] == -1).all())
    assert torch.equal((rank == 0)[rows], ((pred == labels) & (labels >= 0))[rows]), "rank 0 <=> predicted"
    return loss, lse, pred, rank


@pytest.mark.parametrize("dtype,V", CASES, ids=_ids(CASES))
def test_kernel_against_fp64_and_exact_integers(dtype, V, cuda):
    """The edge rows of the loss-option tests, with +1e4 in the pad columns and
    the row maximum in the last real column of row 8."""
    hip.require()
    x, labels, Vp = _edge_rows(dtype, V, 0, cuda)
    x[8, V - 1] = x[8, :V].float().max() + 5
    if Vp > V:
        x[:, V:] = 1e4
    assert bool((labels == -100).any())
    for eps, zeta in OPTIONS:
        _, _, pred, _ = _check(x, labels, V, eps, zeta, f"{dtype} V={V} eps={eps} zeta={zeta}")
        assert int(pred[8]) == V - 1


TIE_CASES = [(dt, V) for dt in (torch.bfloat16, torch.float32) for V in (50257, 128256)]


@pytest.mark.parametrize("dtype,V", TIE_CASES, ids=_ids(TIE_CASES))
def test_tie_rows(dtype, V, cuda):
    hip.require()
    Vp = (V + 63) // 64 * 64
    x, labels = tie_rows(V, Vp, dtype, cuda, threads=THREADS)
    for eps, zeta in OPTIONS[::2]:
        _, _, pred, rank = _check(x, labels, V, eps, zeta, f"ties {dtype} V={V} eps={eps}")
    assert pred[:3].tolist() == [7, 7, 7] and rank[:3].tolist() == [0, 1, 3]  # the {7, 8} set: first, last, duplicate
    assert pred[-3:-1].tolist() == [V // 4, V // 4] and rank[-3:-1].tolist() == [0, 1]  # -0.0 before +0.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bfloat16", "float32"])
def test_non_finite_rows(dtype, cuda):
    """A -inf block (masked vocabulary) is ordinary input.  NaN and +inf are
    tolerated: the prediction stays a column of the row and the other rows of
    the launch are unaffected."""
    hip.require()
    torch.manual_seed(5)
    V, Vp, N = 50257, 50304, 12
    x = (2 * torch.randn(N, Vp, device=cuda)).to(dtype)
    x[:, V:] = 1e4
    labels = torch.randint(0, V, (N,), device=cuda)
    x[0, 1000:20000] = float("-inf")
    labels[0] = 30000
    x[1, :40000] = float("-inf")  # whole threads see nothing finite
    labels[1] = 45000
    x[2, 5] = float("nan")
    x[3, 7] = float("inf")
    x[4] = float("nan")
    x[5] = float("-inf")
    bad = [2, 3, 4, 5]
    good = [i for i in range(N) if i not in bad]
    for eps, zeta in [(0.0, 0.0), (0.0, 1e-3)]:
        _, _, pred, _ = _check(x, labels, V, eps, zeta, f"non-finite {dtype} zeta={zeta}", rows=good)
        assert bool(((pred >= 0) & (pred < V)).all()), pred.tolist()
    torch.cuda.synchronize()


def test_op_on_exact_integer_operands(cuda):
    """h and W hold integers in [-2, 2]: |h . w| <= 256 is exact in bf16 whatever
    GEMM runs, ties are everywhere, and pred / rank have one right answer."""
    hip.require()
    torch.manual_seed(7)
    V, C = 50257, 64
    h = torch.randint(-2, 3, (2, 64, C), device=cuda).bfloat16()
    w = torch.randint(-2, 3, (V, C), device=cuda).bfloat16()
    labels = torch.randint(0, V, (2, 64), device=cuda)
    labels[0, :5] = -100
    logits = h.double().view(-1, C) @ w.double().t()
    assert logits.abs().max().item() <= 256
    with torch.no_grad():
        s = fused.lm_head_score(h, w, labels)
        ce = fused.lm_head_cross_entropy(h, w, labels)
    ref_loss, ref_lse, ref_pred, ref_rank = reference_score(logits, labels.view(-1), V)
    assert torch.equal(s.pred.long().view(-1), ref_pred) and torch.equal(s.rank.long().view(-1), ref_rank)
    assert s.pred.shape == labels.shape and s.rank.shape == labels.shape
    ties = (logits == logits.max(-1, keepdim=True).values).sum(-1)
    assert int(ties.max()) > 1, "the case is meant to have tied maxima"
    nm.assert_elems_close(s.row_loss, ref_loss, 1e-5, 1e-5, "op row loss")
    nm.assert_elems_close(s.lse, ref_lse, 1e-5, 1e-5, "op lse")
    ref = (ref_loss.sum() / (labels != -100).sum()).item()
    print(f"[op] loss {s.loss.item():.7f} fused CE {ce.item():.7f} fp64 {ref:.7f}")
    assert abs(s.loss.item() - ce.item()) <= 2 * (1e-5 * abs(ref) + 1e-5)
    with pytest.raises(RuntimeError, match="forward-only"):
        fused.lm_head_score(h.clone().requires_grad_(), w, labels)


def _models():
    qwen3 = transformers.Qwen3Config(vocab_size=256, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                                     num_attention_heads=2, num_key_value_heads=1, head_dim=128,
                                     max_position_embeddings=512, tie_word_embeddings=False)
    return {
        "llama-512": lambda: L.LlamaForCausalLM(L.llama_config("llama-tiny")),
        "llama-50257": lambda: L.LlamaForCausalLM(L.llama_config("llama-tiny", vocab_size=50257, hidden_size=256)),
        "gpt2": lambda: GPT2LMHeadModel(gpt2_config("gpt2-tiny", n_embd=128, n_head=2)),
        "qwen3": lambda: L.Qwen3ForCausalLM(qwen3),
    }


@pytest.mark.parametrize("kind", ["llama-512", "llama-50257", "gpt2", "qwen3"])
def test_models_predictions_against_default_eval(kind, cuda):
    hip.require()
    torch.manual_seed(0)
    model = _models()[kind]().to(device=cuda, dtype=torch.bfloat16).eval()
    V = model.config.vocab_size
    ids = torch.randint(0, V, (2, 64), device=cuda)

    def close(a, b):
        print(f"[{kind}] loss {a.item():.7f} against {b.item():.7f}")
        return abs(a.item() - b.item()) <= 2 * (1e-5 * abs(b.item()) + 1e-5)

    with torch.no_grad():
        ref = model(ids, labels=ids)
        out = model(ids, labels=ids, predictions=True)
    assert out.logits is None and close(out.loss, ref.loss)
    assert out.predictions.shape == ids.shape and out.label_ranks.shape == ids.shape
    lg = ref.logits.float()
    top = lg.max(-1).values
    got = lg.gather(-1, out.predictions.long()[..., None])[..., 0]
    # the two head GEMMs each round to bf16: one ulp each, two bf16 ulps are at most 2^-6 relative
    assert bool((got >= top - 2.0 ** -6 * top.abs()).all()), (top - got).max().item()
    assert torch.equal(out.label_ranks[:, :-1] == 0, out.predictions[:, :-1] == ids[:, 1:])
    assert bool((out.label_ranks[:, -1] == -1).all()) and bool((out.label_ranks[:, :-1] >= 0).all())
    model.set_loss_options(label_smoothing=0.1)
    with torch.no_grad():
        smooth = model(ids, labels=ids)
        assert close(model(ids, labels=ids, predictions=True).loss, smooth.loss)
    assert smooth.loss.item() != ref.loss.item()  # the smoothing is not a no-op (small at a random init)
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model(ids, labels=ids, predictions=True)
