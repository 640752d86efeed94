"""Label smoothing and z-loss of the fused LM-head cross-entropy off the GPU:
the formula against fp64 autograd, native models against stock HF +
``LabelSmoother``, the trainers' routing, the entry points, validation.

    loss_row = lse - (1 - eps) x_y - eps mean_{j<V}(x_j) + zeta lse^2
"""
import json
import os
import sys

import pytest
import torch
import transformers
from transformers.trainer_pt_utils import LabelSmoother

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from distributed_lion_pytorch_amd.models.gpt2 import GPT2LMHeadModel, gpt2_config  # noqa: E402
from distributed_lion_pytorch_amd.models.llama import LlamaForCausalLM, llama_config  # noqa: E402
from distributed_lion_pytorch_amd.ops import fused  # noqa: E402

EPS = 0.1
V, T = 101, 16


def _rel(a, b):
    return (a.double() - b.double()).abs().max().item() / b.double().abs().max().item()


# ------------------------------------------------------------ 1. fp64 oracle
@pytest.mark.parametrize("z", [0.0, 1e-3])
@pytest.mark.parametrize("normalizer", [None, 23.0])
def test_loss_and_gradients_against_fp64_autograd(z, normalizer):
    torch.manual_seed(0)
    B, Tn, C = 2, 9, 16
    h = torch.randn(B, Tn, C, requires_grad=True)
    w = (0.5 * torch.randn(V, C)).requires_grad_()
    labels = torch.randint(0, V, (B, Tn))
    labels[0, :2] = -100
    labels[1, 5] = -100
    loss = fused.lm_head_cross_entropy(h, w, labels, normalizer=normalizer, label_smoothing=EPS, z_loss=z)
    dh, dw = torch.autograd.grad(loss, (h, w))

    h64, w64 = h.detach().double().requires_grad_(), w.detach().double().requires_grad_()
    x = (h64 @ w64.t()).view(-1, V)
    lab = labels.view(-1)
    valid = lab != -100
    lse = torch.logsumexp(x, -1)
    row = lse - (1 - EPS) * x.gather(1, lab.clamp_min(0)[:, None])[:, 0] - EPS * x.mean(-1) + z * lse * lse
    ref = (row * valid).sum() / (valid.sum() if normalizer is None else normalizer)
    rh, rw = torch.autograd.grad(ref, (h64, w64))
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    assert _rel(dh, rh) <= 1e-5 and _rel(dw, rw) <= 1e-5
    if z == 0.0 and normalizer is None:  # and this is F.cross_entropy's label smoothing
        ce = torch.nn.functional.cross_entropy(x, lab, ignore_index=-100, label_smoothing=EPS)
        assert abs(ce.item() - ref.item()) < 1e-12


# ------------------------------------------------------------ 2. native models vs stock HF
def _tiny_pair(kind, tmp_path):
    torch.manual_seed(0)
    if kind == "gpt2":
        cfg = gpt2_config("gpt2-tiny", vocab_size=V, bos_token_id=V - 1, eos_token_id=V - 1, resid_pdrop=0.0,
                          embd_pdrop=0.0, attn_pdrop=0.0)
        ours, hf_cls = GPT2LMHeadModel(cfg), transformers.GPT2LMHeadModel
    else:
        cfg = llama_config("llama-tiny", hidden_size=64, intermediate_size=128, vocab_size=V)
        ours, hf_cls = LlamaForCausalLM(cfg), transformers.LlamaForCausalLM
    assert cfg.num_hidden_layers == 2 and cfg.hidden_size == 64
    ours.save_pretrained(tmp_path)
    return ours, hf_cls.from_pretrained(tmp_path)


def _batch():
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, V, (3, T), generator=g)
    labels = ids.clone()
    labels[0, :4] = -100
    return ids, labels


@pytest.mark.parametrize("num_items", [None, 37])
@pytest.mark.parametrize("kind", ["gpt2", "llama"])
def test_native_models_match_hf_label_smoother(kind, num_items, tmp_path):
    ours, hf = _tiny_pair(kind, tmp_path)
    ours.set_loss_options(label_smoothing=EPS)
    ids, labels = _batch()
    n = None if num_items is None else torch.tensor(num_items)
    la = ours(ids, labels=labels, num_items_in_batch=n).loss
    lb = LabelSmoother(EPS)(hf(ids), labels, shift_labels=True, num_items_in_batch=n)
    assert abs(la.item() - lb.item()) < 1e-5
    # the smoothing is not a no-op here (small at a random init, whose logits are nearly uniform)
    assert abs(la.item() - hf(ids, labels=labels).loss.item()) > 1e-4
    la.backward()
    lb.backward()
    for (na, pa), (nb, pb) in zip(ours.named_parameters(), hf.named_parameters()):
        assert na == nb
        assert (pa.grad - pb.grad).abs().max().item() < 1e-5, na


def test_z_loss_only_in_training_smoothing_also_in_eval(tmp_path):
    ours, hf = _tiny_pair("llama", tmp_path)
    ids, labels = _batch()
    ours.set_loss_options(label_smoothing=EPS, z_loss=1e-2)
    smoothed = LabelSmoother(EPS)(hf(ids), labels, shift_labels=True).item()
    ours.eval()
    assert abs(ours(ids, labels=labels).loss.item() - smoothed) < 1e-5
    ours.train()
    lse = torch.logsumexp(hf(ids).logits[:, :-1].double(), -1)[labels[:, 1:] != -100]
    want = smoothed + 1e-2 * (lse * lse).mean().item()
    assert abs(ours(ids, labels=labels).loss.item() - want) < 1e-5


def test_options_are_not_saved(tmp_path):
    ours, _ = _tiny_pair("gpt2", tmp_path / "a")
    before = json.load(open(tmp_path / "a" / "config.json"))
    ours.set_loss_options(label_smoothing=EPS, z_loss=1e-3)
    ours.save_pretrained(tmp_path / "b")
    assert json.load(open(tmp_path / "b" / "config.json")) == before
    assert not hasattr(ours.config, "label_smoothing") and not hasattr(ours.config, "z_loss")
    transformers.GPT2LMHeadModel.from_pretrained(tmp_path / "b")  # stock HF still loads it


# ------------------------------------------------------------ 3. trainer routing
def _trainer(model, out_dir, **kw):
    from distributed_lion_pytorch_amd.trainer.async_trainer import AsyncTrainer, AsyncTrainingArguments

    ids, labels = _batch()
    data = [{"input_ids": ids[i], "labels": labels[i]} for i in range(ids.shape[0])]
    args = AsyncTrainingArguments(output_dir=str(out_dir), use_cpu=True, max_steps=1, per_device_train_batch_size=3,
                                  learning_rate=1e-3, async_grad=True, report_to="none", save_strategy="no",
                                  dataloader_num_workers=0, label_smoothing_factor=EPS, **kw)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    return AsyncTrainer(model=model, args=args, train_dataset=data, optimizers=(opt, None))


def test_trainer_routes_label_smoothing_into_the_native_model(tmp_path):
    ours, hf = _tiny_pair("gpt2", tmp_path / "m")
    tr = _trainer(ours, tmp_path / "o", lm_z_loss=0.0)
    assert tr.label_smoother is None
    assert ours.label_smoothing == pytest.approx(EPS) and ours.z_loss == 0.0
    seen = {}
    forward = ours.forward

    def spy(*a, **kw):
        seen.update(kw)
        return forward(*a, **kw)

    ours.forward = spy
    ids, labels = _batch()
    tr.current_gradient_accumulation_steps = 1
    loss = tr.training_step(tr.model, {"input_ids": ids, "labels": labels})
    assert seen.get("labels") is not None, "the labels must reach the model's fused loss"
    want = LabelSmoother(EPS)(hf(ids), labels, shift_labels=True)
    assert abs(loss.item() - want.item()) < 1e-5


def test_trainer_sets_z_loss_and_keeps_hf_smoother_for_stock_models(tmp_path):
    ours, hf = _tiny_pair("gpt2", tmp_path / "m")
    tr = _trainer(ours, tmp_path / "o", lm_z_loss=1e-4)
    assert tr.label_smoother is None and ours.z_loss == pytest.approx(1e-4)
    state = {k: v.clone() for k, v in hf.state_dict().items()}
    tr_hf = _trainer(hf, tmp_path / "p")
    assert isinstance(tr_hf.label_smoother, LabelSmoother) and tr_hf.label_smoother.epsilon == pytest.approx(EPS)
    assert not hasattr(hf, "label_smoothing") and not hasattr(hf, "set_loss_options")
    assert all(torch.equal(v, state[k]) for k, v in hf.state_dict().items())
    with pytest.raises(ValueError, match="lm_z_loss"):
        _trainer(hf, tmp_path / "q", lm_z_loss=1e-4)


def test_lora_injected_native_model_counts_as_native(tmp_path):
    from distributed_lion_pytorch_amd.models.lora import LoraConfig, inject_lora

    ours, _ = _tiny_pair("llama", tmp_path / "m")
    inject_lora(ours, LoraConfig(r=4, lora_alpha=8, target_modules=["q_proj", "v_proj"]))
    tr = _trainer(ours, tmp_path / "o", lm_z_loss=1e-4)
    assert tr.label_smoother is None
    assert ours.label_smoothing == pytest.approx(EPS) and ours.z_loss == pytest.approx(1e-4)


# ------------------------------------------------------------ 4. entry points
def test_run_clm_with_label_smoothing_and_z_loss(tmp_path):
    import run_clm

    out = str(tmp_path / "clm")
    trainer = run_clm.main(["--synthetic_data", "--synthetic_samples", "32", "--block_size", "32",
                            "--per_device_train_batch_size", "4", "--warmup_steps", "1", "--learning_rate", "1e-3",
                            "--report_to", "none", "--use_cpu", "--logging_steps", "1", "--config_name", "gpt2-tiny",
                            "--max_steps", "2", "--lion", "--async_grad", "--do_train", "--output_dir", out,
                            "--label_smoothing_factor", "0.1", "--lm_z_loss", "1e-4"])
    assert trainer.label_smoother is None
    assert trainer.model.label_smoothing == pytest.approx(0.1) and trainer.model.z_loss == pytest.approx(1e-4)
    recs = [json.loads(x) for x in open(os.path.join(out, "metrics.jsonl"))]
    assert sum("loss" in r for r in recs) >= 2
    saved = json.load(open(os.path.join(out, "config.json")))
    plain = gpt2_config("gpt2-tiny").to_dict()
    assert set(saved) <= set(plain) | {"architectures", "dtype", "torch_dtype", "transformers_version"}, \
        sorted(set(saved) - set(plain))
    assert not any("smooth" in k or "z_loss" in k for k in saved)


def test_dpo_refuses_lm_z_loss(tmp_path):
    import dpo_llama2

    with pytest.raises(SystemExit, match="lm_z_loss"):
        dpo_llama2.main(["--model_name_or_path", "llama-tiny", "--synthetic_data", "--output_dir", str(tmp_path),
                         "--use_cpu", "--lm_z_loss", "1e-4"])


# ------------------------------------------------------------ 5. validation and defaults
@pytest.mark.parametrize("kw", [{"label_smoothing": -0.1}, {"label_smoothing": 1.0}, {"label_smoothing": float("nan")},
                                {"z_loss": -1e-3}, {"z_loss": float("nan")}])
def test_out_of_range_options_raise(kw):
    h, w, labels = torch.randn(4, 8), torch.randn(11, 8), torch.randint(0, 11, (4,))
    with pytest.raises(ValueError):
        fused.lm_head_cross_entropy(h, w, labels, **kw)
    with pytest.raises(ValueError):
        fused.causal_lm_loss(h[None], w, labels[None], **kw)
    m = GPT2LMHeadModel(gpt2_config("gpt2-tiny"))
    with pytest.raises(ValueError):
        m.set_loss_options(**kw)


def test_zero_options_are_bit_identical_to_the_plain_call():
    torch.manual_seed(1)
    h0, w0 = torch.randn(2, 9, 16), 0.5 * torch.randn(V, 16)
    labels = torch.randint(0, V, (2, 9))
    labels[1, 0] = -100
    out = []
    for kw in ({}, {"label_smoothing": 0.0, "z_loss": 0.0}):
        h, w = h0.clone().requires_grad_(), w0.clone().requires_grad_()
        loss = fused.lm_head_cross_entropy(h, w, labels, **kw)
        loss.backward()
        out.append((loss.detach(), h.grad, w.grad))
    for a, b in zip(*out):
        assert torch.equal(a, b)
