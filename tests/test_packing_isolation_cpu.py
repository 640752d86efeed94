"""Document-isolated packing off the GPU: the visibility bounds, the math-SDPA
fallback, the Llama model against HF run per document, the packing datasets
and the sft_llama2 entrypoint."""
import json
import math
import os
import sys
import tempfile

import pytest
import torch
import transformers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from distributed_lion_pytorch_amd.models.llama import LlamaForCausalLM, llama_config  # noqa: E402
from distributed_lion_pytorch_amd.ops import fused  # noqa: E402
from distributed_lion_pytorch_amd.utils.data import (ByteTokenizer, ConstantLengthDataset, PackedStream,  # noqa: E402
                                                     prepare_sample_text, synthetic_qa)


def _position_ids(docs):
    return torch.cat([torch.arange(n) for n in docs])


def _spans(docs):
    out, s = [], 0
    for n in docs:
        out.append((s, s + n))
        s += n
    return out


# ------------------------------------------------------------ visibility_bounds
DOCS100 = [1, 31, 32, 33, 3]  # boundaries at 1, 32, 64, 97


def _expected_bounds(docs, window):
    """row_lo / key_hi from their definitions, one Python loop per document."""
    T = sum(docs)
    lo, hi = [0] * T, [0] * T
    for s, e in _spans(docs):
        for t in range(s, e):
            lo[t], hi[t] = s, e
            if 0 < window < T:
                lo[t], hi[t] = max(s, t - window + 1), min(e, t + window)
    return lo, hi


def test_visibility_bounds_t100_exact():
    pos = torch.stack([_position_ids(DOCS100), torch.arange(100)])
    row_lo, key_hi = fused.visibility_bounds(pos)
    assert row_lo.dtype == key_hi.dtype == torch.int32 and row_lo.shape == key_hi.shape == (2, 100)
    assert row_lo.is_contiguous() and key_hi.is_contiguous()
    # around every boundary: the last token of a document, the first of the next
    at = [0, 1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 98, 99]
    assert row_lo[0, at].tolist() == [0, 1, 1, 1, 32, 32, 32, 64, 64, 64, 97, 97, 97]
    assert key_hi[0, at].tolist() == [1, 32, 32, 32, 64, 64, 64, 97, 97, 97, 100, 100, 100]
    lo, hi = _expected_bounds(DOCS100, 0)
    assert row_lo[0].tolist() == lo and key_hi[0].tolist() == hi
    # the unsegmented row is plain causal
    assert row_lo[1].tolist() == [0] * 100 and key_hi[1].tolist() == [100] * 100


def test_visibility_bounds_t100_window16_exact():
    pos = torch.stack([_position_ids(DOCS100), torch.arange(100)])
    row_lo, key_hi = fused.visibility_bounds(pos, 16)
    at = [0, 1, 16, 17, 31, 32, 47, 48, 63, 64, 79, 80, 96, 97, 99]
    # row_lo = max(document start, q - 15)
    assert row_lo[0, at].tolist() == [0, 1, 1, 2, 16, 32, 32, 33, 48, 64, 64, 65, 81, 97, 97]
    # key_hi = min(next document start, k + 16)
    assert key_hi[0, at].tolist() == [1, 17, 32, 32, 32, 48, 63, 64, 64, 80, 95, 96, 97, 100, 100]
    lo, hi = _expected_bounds(DOCS100, 16)
    assert row_lo[0].tolist() == lo and key_hi[0].tolist() == hi
    assert row_lo[1].tolist() == [max(0, t - 15) for t in range(100)]
    assert key_hi[1].tolist() == [min(100, t + 16) for t in range(100)]
    # both views describe one relation, and both are non-decreasing
    for b in range(2):
        for kk in range(100):
            seen_by = [q for q in range(100) if int(row_lo[b, q]) <= kk <= q]
            assert seen_by == list(range(kk, int(key_hi[b, kk])))
        assert (row_lo[b, 1:] >= row_lo[b, :-1]).all() and (key_hi[b, 1:] >= key_hi[b, :-1]).all()
    # a window covering the row changes nothing
    a, b_ = fused.visibility_bounds(pos, 100)
    c, d = fused.visibility_bounds(pos)
    assert torch.equal(a, c) and torch.equal(b_, d)


def test_visibility_bounds_rejects_a_jump_inside_a_document():
    pos = _position_ids([5, 7])[None].clone()
    fused.visibility_bounds(pos)  # fine
    pos[0, 8] = 9  # 0 1 2 | 9
    with pytest.raises(ValueError, match="position_ids"):
        fused.visibility_bounds(pos)
    rep = torch.tensor([[0, 1, 1, 2]])  # a repeated position
    with pytest.raises(ValueError, match="position_ids"):
        fused.visibility_bounds(rep)


# ------------------------------------------------------------ fallback attention
def _per_document(fn, q, k, v, docs, *tables):
    outs = []
    for s, e in _spans(docs):
        outs.append(fn(q[:, s:e], k[:, s:e], v[:, s:e], *(t[s:e] for t in tables)))
    return torch.cat(outs, dim=1)


@pytest.mark.parametrize("docs,window", [([7, 20, 13], 0), ([1, 12, 1, 26], 0), ([25, 15], 8)])
def test_fallback_attention_with_bounds_equals_per_document_calls(docs, window):
    """fp64 on the CPU (math SDPA): causal_attention_gqa and rope_attention with
    bounds equal the per-document calls concatenated, gradients included.  The
    rotary tables keep the global positions in both."""
    torch.manual_seed(0)
    B, T, H, Hkv, D = 2, sum(docs), 4, 2, 16
    q, k, v = (torch.randn(B, T, h, D, dtype=torch.float64) for h in (H, Hkv, Hkv))
    dout = torch.randn(B, T, H * D, dtype=torch.float64)
    ang = torch.arange(T, dtype=torch.float64)[:, None] * (10000.0 ** (-torch.arange(0, D, 2, dtype=torch.float64) / D))
    cos, sin = torch.cat([ang.cos(), ang.cos()], -1), torch.cat([ang.sin(), ang.sin()], -1)
    bounds = fused.visibility_bounds(_position_ids(docs)[None].expand(B, T), window)
    for name, full, part, tables in (
            ("gqa", lambda a, b, c: fused.causal_attention_gqa(a, b, c, 0.0, window, bounds),
             lambda a, b, c: fused.causal_attention_gqa(a, b, c, 0.0, window), ()),
            ("rope", lambda a, b, c: fused.rope_attention(a, b, c, cos, sin, 0.0, window, bounds),
             lambda a, b, c, cs, sn: fused.rope_attention(a, b, c, cs, sn, 0.0, window), (cos, sin))):
        a = [t.clone().requires_grad_() for t in (q, k, v)]
        r = [t.clone().requires_grad_() for t in (q, k, v)]
        out = full(*a)
        ref = _per_document(part, *r, docs, *tables)
        torch.testing.assert_close(out, ref, msg=lambda m: f"{name} out: {m}")
        out.backward(dout)
        ref.backward(dout)
        for x, y, n in zip(a, r, "qkv"):
            torch.testing.assert_close(x.grad, y.grad, msg=lambda m: f"{name} d{n}: {m}")


# ------------------------------------------------------------------------ model
def _grads_close(a, b, tol=1e-5):
    for (na, pa), (nb, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert na == nb
        if pa.grad is None and pb.grad is None:
            continue
        assert (pa.grad - pb.grad).abs().max().item() < tol, na


def hf_per_document_loss(hf, ids, docs):
    """Token-weighted mean of HF's loss over each document run alone (a
    document of n tokens has n - 1 predictions)."""
    total, count = 0.0, 0
    for b in range(ids.shape[0]):
        for s, e in _spans(docs):
            if e - s < 2:
                continue
            x = ids[b:b + 1, s:e]
            total = total + hf(x, labels=x).loss * (e - s - 1)
            count += e - s - 1
    return total / count


def test_llama_with_position_ids_matches_hf_run_per_document():
    cfg = llama_config("llama-tiny")
    torch.manual_seed(0)
    ours = LlamaForCausalLM(cfg)
    with tempfile.TemporaryDirectory() as d:
        ours.save_pretrained(d)
        hf = transformers.LlamaForCausalLM.from_pretrained(d)
    docs = [7, 20, 13]
    ids = torch.randint(0, cfg.vocab_size, (1, sum(docs)))
    pos = _position_ids(docs)[None]
    labels = ids.clone()
    labels[pos == 0] = -100
    la = ours(ids, labels=labels, position_ids=pos).loss
    lb = hf_per_document_loss(hf, ids, docs)
    assert abs(la.item() - lb.item()) < 1e-5, (la.item(), lb.item())
    la.backward()
    lb.backward()
    _grads_close(ours, hf)
    # without position_ids the same labels give the cross-document loss: the test can fail
    with torch.no_grad():
        leak = ours(ids, labels=labels).loss
    assert abs(leak.item() - lb.item()) > 1e-3, (leak.item(), lb.item())


# --------------------------------------------------------------------- datasets
def _check_isolated_items(items, plain, eos):
    assert len(items) == len(plain) and len(items) > 1
    n_restarts = 0
    for it, pl in zip(items, plain):
        assert set(pl) == {"input_ids", "labels"}
        assert torch.equal(it["input_ids"], pl["input_ids"])
        ids, pos, labels = it["input_ids"], it["position_ids"], it["labels"]
        assert pos.dtype == torch.long and pos.shape == ids.shape
        assert int(pos[0]) == 0  # a block starts a document, also when it cuts a sample
        for t in range(1, len(ids)):
            if int(ids[t - 1]) == eos:  # the EOS is the last token of its document
                assert int(pos[t]) == 0, t
                n_restarts += 1
            else:
                assert int(pos[t]) == int(pos[t - 1]) + 1, t
        assert torch.equal(labels == -100, pos == 0)
        assert torch.equal(labels[pos != 0], ids[pos != 0])
        fused.visibility_bounds(pos[None])  # a valid input of the attention op
    assert n_restarts > 0


def test_packing_datasets_isolate_documents():
    tok = ByteTokenizer()
    rows = synthetic_qa(40, seed=3)
    on = ConstantLengthDataset(tok, rows, prepare_sample_text, seq_length=96, isolate_documents=True)
    off = ConstantLengthDataset(tok, rows, prepare_sample_text, seq_length=96)
    _check_isolated_items([on[i] for i in range(len(on))], [off[i] for i in range(len(off))], tok.eos_token_id)
    kw = dict(seq_length=96, infinite=False, chars_per_token=1.0, num_of_sequences=4, shard=False)
    on = list(PackedStream(tok, rows, prepare_sample_text, isolate_documents=True, **kw))
    off = list(PackedStream(tok, rows, prepare_sample_text, **kw))
    _check_isolated_items(on, off, tok.eos_token_id)


def test_sft_trainer_passes_isolate_documents_to_the_datasets_it_builds(tmp_path):
    from transformers import TrainingArguments

    from distributed_lion_pytorch_amd.trainer.sft import SFTTrainer

    cfg = llama_config("llama-tiny")
    model = LlamaForCausalLM(cfg)
    args = TrainingArguments(output_dir=str(tmp_path), report_to="none", use_cpu=True, max_steps=1)
    rows = synthetic_qa(12, seed=1)
    tr = SFTTrainer(model=model, args=args, train_dataset=rows, tokenizer=ByteTokenizer(), max_seq_length=64,
                    isolate_documents=True)
    assert "position_ids" in tr.train_dataset[0]
    tr = SFTTrainer(model=model, args=args, train_dataset=rows, tokenizer=ByteTokenizer(), max_seq_length=64)
    assert "position_ids" not in tr.train_dataset[0]


# ------------------------------------------------------------------- entrypoint
SFT_ARGS = ["--synthetic_data", "--synthetic_samples", "100", "--seq_length", "64", "--max_steps", "2",
            "--per_device_train_batch_size", "2", "--learning_rate", "1e-3", "--lion", "--async_grad", "--report_to",
            "none", "--use_cpu", "--torch_dtype", "float32", "--logging_steps", "1", "--final_save", "false"]


def test_sft_llama2_isolate_documents_trains(tmp_path):
    import sft_llama2

    out = str(tmp_path / "iso")
    tr = sft_llama2.main(["--model_name", "llama-tiny", "--output_dir", out, "--isolate_documents"] + SFT_ARGS)
    assert tr.state.global_step == 2
    batch = next(iter(tr.get_train_dataloader()))
    assert "position_ids" in batch and batch["position_ids"].shape == batch["input_ids"].shape
    assert torch.equal(batch["labels"] == -100, batch["position_ids"] == 0)
    with open(os.path.join(out, "metrics.jsonl")) as f:
        recs = [json.loads(line) for line in f]
    losses = [r["loss"] for r in recs if "loss" in r]
    assert losses and all(math.isfinite(x) for x in losses), recs


def test_sft_llama2_default_batches_have_no_position_ids(tmp_path):
    import sft_llama2

    tr = sft_llama2.main(["--model_name", "llama-tiny", "--output_dir", str(tmp_path / "plain")] + SFT_ARGS)
    batch = next(iter(tr.get_train_dataloader()))
    assert "position_ids" not in batch


def test_sft_llama2_isolate_documents_refuses_a_non_native_model(tmp_path):
    import sft_llama2

    neox = transformers.GPTNeoXConfig(vocab_size=300, hidden_size=64, num_hidden_layers=1, num_attention_heads=4,
                                      intermediate_size=128)
    transformers.GPTNeoXForCausalLM(neox).save_pretrained(tmp_path / "neox")  # the stock-HF fallback of build_model
    with pytest.raises(ValueError, match="needs a native Llama-family model"):
        sft_llama2.main(["--model_name", str(tmp_path / "neox"), "--output_dir", str(tmp_path / "o"),
                         "--isolate_documents"] + SFT_ARGS)
    # GPT-2 is native but has no document isolation either
    with pytest.raises(ValueError, match="needs a native Llama-family model"):
        sft_llama2.main(["--model_name", "gpt2-tiny", "--output_dir", str(tmp_path / "o2"),
                         "--isolate_documents"] + SFT_ARGS)
