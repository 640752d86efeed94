"""Evaluation without logits, on the CPU: the PyTorch form of the scoring op
against fp64 on tie rows, ``predictions=True`` on fp32 native models against
``logits.argmax``, ``token_predictions`` on a logits tensor, the trainers'
``ScoredEvalMixin`` routing, and ``run_clm.py --do_eval`` metrics."""
import functools
import json
import os

import pytest
import torch
import torch.nn.functional as F

from distributed_lion_pytorch_amd import token_predictions
from distributed_lion_pytorch_amd.models.gpt2 import GPT2LMHeadModel, gpt2_config
from distributed_lion_pytorch_amd.models.llama import LlamaForCausalLM, llama_config
from distributed_lion_pytorch_amd.ops import fused
from lm_score_cases import reference_score, tie_rows

V, T = 97, 24


# ------------------------------------------------------------ 1. the PyTorch form
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("v", [100, 512])
def test_lm_score_torch_against_fp64_on_tie_rows(v, dtype):
    vp = 128 if v == 100 else 576  # garbage in the pad columns, larger than every real value
    x, labels = tie_rows(v, vp, dtype, torch.device("cpu"), threads=4)
    keep = x.clone()
    for eps, zeta in [(0.0, 0.0), (0.1, 0.0), (0.1, 1e-3)]:
        loss, lse, pred, rank = fused._lm_score_torch(x, labels, v, eps, zeta)
        ref_loss, ref_lse, ref_pred, ref_rank = reference_score(x, labels, v, eps, zeta)
        assert pred.dtype == torch.int32 and rank.dtype == torch.int32 and loss.dtype == torch.float32
        assert torch.equal(pred.long(), ref_pred) and torch.equal(rank.long(), ref_rank)
        assert (loss.double() - ref_loss).abs().max().item() <= 1e-5 * ref_loss.abs().max().item() + 1e-5
        assert (lse.double() - ref_lse).abs().max().item() <= 1e-5 * ref_lse.abs().max().item() + 1e-5
        assert torch.equal(rank == 0, (pred == labels) & (labels >= 0))
        assert loss[labels < 0].abs().max().item() == 0.0 and bool((rank[labels < 0] == -1).all())
    assert torch.equal(x, keep)


def test_lm_head_score_is_forward_only():
    h = torch.randn(2, 5, 16, requires_grad=True)
    w = torch.randn(V, 16)
    labels = torch.randint(0, V, (2, 5))
    with pytest.raises(RuntimeError, match="forward-only"):
        fused.lm_head_score(h, w, labels)
    with torch.no_grad():
        s = fused.lm_head_score(h, w, labels, label_smoothing=0.1, z_loss=1e-3)
        want = fused.lm_head_cross_entropy(h, w, labels, label_smoothing=0.1, z_loss=1e-3)
    assert not s.loss.requires_grad and s.pred.shape == labels.shape and s.rank.shape == labels.shape
    assert abs(s.loss.item() - want.item()) < 1e-5


# ------------------------------------------------------------ 2. fp32 models
def _tiny(kind):
    torch.manual_seed(0)
    if kind == "gpt2":
        cfg = gpt2_config("gpt2-tiny", vocab_size=V, bos_token_id=V - 1, eos_token_id=V - 1)
        return GPT2LMHeadModel(cfg).eval()
    return LlamaForCausalLM(llama_config("llama-tiny", hidden_size=64, intermediate_size=128, vocab_size=V)).eval()


def _batch():
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, V, (3, T), generator=g)
    labels = ids.clone()
    labels[0, :4] = -100
    return ids, labels


@pytest.mark.parametrize("kind", ["gpt2", "llama"])
def test_predictions_equal_argmax_in_fp32(kind):
    model = _tiny(kind)
    ids, labels = _batch()
    with torch.no_grad():
        ref = model(ids, labels=labels)
        out = model(ids, labels=labels, predictions=True)
    top2 = ref.logits.topk(2, dim=-1).values
    assert (top2[..., 0] - top2[..., 1]).min().item() > 1e-4, "precondition: choose a seed without near-ties"
    assert out.logits is None and out.predictions.shape == ids.shape and out.label_ranks.shape == ids.shape
    assert torch.equal(out.predictions.long(), ref.logits.argmax(-1))
    assert abs(out.loss.item() - ref.loss.item()) < 1e-5
    shifted = fused.shift_labels(labels)
    want = (ref.logits > ref.logits.gather(-1, shifted.clamp_min(0)[..., None])).sum(-1)
    assert torch.equal(out.label_ranks.long(), torch.where(shifted >= 0, want, torch.full_like(want, -1)))
    assert bool((out.label_ranks[:, -1] == -1).all()) and bool((out.label_ranks[0, :3] == -1).all())
    # token_predictions on the logits of a model without the scoring path: the same pair
    pred, rank = token_predictions(ref.logits, labels)
    assert torch.equal(pred, out.predictions) and torch.equal(rank, out.label_ranks)
    assert token_predictions((out.predictions, out.label_ranks), labels) == (out.predictions, out.label_ranks)
    # label smoothing reaches the scored loss as it reaches the evaluation loss
    model.set_loss_options(label_smoothing=0.1, z_loss=1e-2)
    with torch.no_grad():
        assert abs(model(ids, labels=labels, predictions=True).loss.item() - model(ids, labels=labels).loss.item()) < 1e-5
    assert abs(model(ids, labels=labels, predictions=True).loss.item() - ref.loss.item()) > 1e-4
    with pytest.raises(ValueError, match="labels"):
        model(ids, predictions=True)
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model(ids, labels=labels, predictions=True)


# ------------------------------------------------------------ 3. trainers
class _Spy:
    """Counts F.linear calls against the LM-head weight and records what the model's forward got and gave."""

    def __init__(self, model, monkeypatch):
        self.head_linears, self.kwargs, self.outputs = 0, [], []
        real_linear, forward, head = F.linear, model.forward, model.lm_head.weight

        def linear(x, w, *a, **kw):
            self.head_linears += w is head
            return real_linear(x, w, *a, **kw)

        @functools.wraps(forward)  # the mixin inspects the forward's signature
        def spy(*a, **kw):
            self.kwargs.append(kw)
            out = forward(*a, **kw)
            self.outputs.append(out)
            return out

        monkeypatch.setattr(F, "linear", linear)
        model.forward = spy


def _trainer(cls, model, out_dir, **kw):
    from distributed_lion_pytorch_amd.trainer.async_trainer import AsyncTrainingArguments

    ids, labels = _batch()
    data = [{"input_ids": ids[i], "labels": labels[i]} for i in range(ids.shape[0])]
    targs = {k: kw.pop(k) for k in list(kw) if k in ("fused_eval",)}
    args = AsyncTrainingArguments(output_dir=str(out_dir), use_cpu=True, per_device_eval_batch_size=2,
                                  report_to="none", save_strategy="no", dataloader_num_workers=0, **targs)
    return cls(model=model, args=args, eval_dataset=data, **kw)


def _metrics(eval_preds):
    (preds, ranks), labels = eval_preds
    mask = labels[:, 1:] != -100
    return {"accuracy": float((preds[:, :-1][mask] == labels[:, 1:][mask]).mean()),
            "top5_accuracy": float((ranks[:, :-1][mask] < 5).mean())}


def test_local_trainer_evaluates_without_logits(tmp_path, monkeypatch):
    from distributed_lion_pytorch_amd.trainer.async_trainer import LocalTrainer

    model = _tiny("gpt2")
    spy = _Spy(model, monkeypatch)
    tr = _trainer(LocalTrainer, model, tmp_path, compute_metrics=_metrics,
                  preprocess_logits_for_metrics=token_predictions)
    m = tr.evaluate()
    assert spy.head_linears == 0 and len(spy.kwargs) == 2
    assert all(kw.get("predictions") is True for kw in spy.kwargs) and all(o.logits is None for o in spy.outputs)
    assert 0.0 <= m["eval_accuracy"] <= m["eval_top5_accuracy"] <= 1.0
    ids, labels = _batch()
    with torch.no_grad():
        ref = model(ids, labels=labels)
    mask = labels[:, 1:] != -100
    want = (ref.logits.argmax(-1)[:, :-1][mask] == labels[:, 1:][mask]).float().mean().item()
    assert m["eval_accuracy"] == pytest.approx(want, abs=1e-7)


@pytest.mark.parametrize("how", ["flag", "user_preprocess"])
def test_logits_path_is_kept_on_request(how, tmp_path, monkeypatch):
    from distributed_lion_pytorch_amd.trainer.async_trainer import LocalTrainer

    model = _tiny("gpt2")
    spy = _Spy(model, monkeypatch)
    if how == "flag":
        tr = _trainer(LocalTrainer, model, tmp_path, compute_metrics=_metrics,
                      preprocess_logits_for_metrics=token_predictions, fused_eval=False)
    else:
        tr = _trainer(LocalTrainer, model, tmp_path, compute_metrics=_metrics,
                      preprocess_logits_for_metrics=lambda logits, labels: token_predictions(logits, labels))
    m = tr.evaluate()
    assert spy.head_linears == 2 and not any(kw.get("predictions") for kw in spy.kwargs)
    assert all(o.logits is not None for o in spy.outputs)
    assert 0.0 <= m["eval_accuracy"] <= m["eval_top5_accuracy"] <= 1.0


def test_loss_only_evaluation_of_the_sft_trainer_is_scored(tmp_path, monkeypatch):
    from distributed_lion_pytorch_amd.trainer.sft import SFTTrainer

    model = _tiny("llama")
    want = _trainer(SFTTrainer, model, tmp_path / "logits", fused_eval=False).evaluate()["eval_loss"]
    spy = _Spy(model, monkeypatch)
    tr = _trainer(SFTTrainer, model, tmp_path / "scored")
    m = tr.evaluate()
    assert len(spy.kwargs) == 2 and spy.head_linears == 0
    assert all(kw.get("predictions") is True for kw in spy.kwargs) and all(o.logits is None for o in spy.outputs)
    assert m["eval_loss"] == pytest.approx(want, abs=1e-5)


# ------------------------------------------------------------ 4. run_clm.py --do_eval
def test_run_clm_reports_accuracy_and_top5(tmp_path):
    import run_clm

    def run(name, extra):
        out = str(tmp_path / name)
        run_clm.main(["--synthetic_data", "--synthetic_samples", "16", "--block_size", "32", "--report_to", "none",
                      "--use_cpu", "--config_name", "gpt2-tiny", "--per_device_eval_batch_size", "4", "--do_eval",
                      "--seed", "5", "--output_dir", out] + extra)
        return json.load(open(os.path.join(out, "eval_results.json")))

    a, b = run("scored", []), run("logits", ["--fused_eval", "False"])
    assert 0.0 <= a["eval_accuracy"] <= a["eval_top5_accuracy"] <= 1.0
    assert a["eval_accuracy"] == b["eval_accuracy"] and a["eval_top5_accuracy"] == b["eval_top5_accuracy"]
    assert a["eval_loss"] == pytest.approx(b["eval_loss"], abs=1e-5)
