#!/usr/bin/env python
"""Generate text with a native model: KV cache + the gfx950 decode-attention kernel.

    python generate.py --model_name_or_path gpt2 --prompt "The quick brown fox" --max_new_tokens 32
    python generate.py --model_name_or_path ./sft/final_merged_checkpoint --prompt_file prompts.txt --bf16 \\
        --do_sample --temperature 0.8 --top_p 0.95 --seed 0
    python generate.py --model_name_or_path llama-2-7b --adapter ./sft/final_checkpoint --prompt "..." --bf16
    python generate.py --model_name_or_path gpt2 --prompt "The quick brown fox" --num_beams 4 --num_return_sequences 2
    python generate.py --model_name_or_path llama-2-7b --load_in_4bit --adapter ./sft/final_checkpoint \\
        --prompt "..." --bf16
    python generate.py --model_name_or_path ./llama-8b --assistant_model ./llama-1b --num_assistant_tokens 5 \\
        --prompt "..." --bf16

``--model_name_or_path`` is a named size (random weights, no hub access) or a local HF directory
(models/registry.py); ``--adapter`` a peft-format LoRA directory as sft_llama2.py writes it.  A directory without a
tokenizer falls back to the byte tokenizer.  Prompts of different lengths run as one left-padded batch.  Prints
the completions and tokens/s.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from distributed_lion_pytorch_amd.models.lora import load_adapter  # noqa: E402
from distributed_lion_pytorch_amd.models.registry import build_model, load_config  # noqa: E402
from distributed_lion_pytorch_amd.utils.data import load_tokenizer  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model_name_or_path", required=True)
    ap.add_argument("--adapter", default=None, help="peft-format LoRA directory (sft_llama2.py's final_checkpoint)")
    ap.add_argument("--prompt", action="append", default=[], help="a prompt (repeatable)")
    ap.add_argument("--prompt_file", default=None, help="one prompt per line")
    ap.add_argument("--max_new_tokens", type=int, default=64)
    ap.add_argument("--do_sample", action="store_true")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top_k", type=int, default=0)
    ap.add_argument("--top_p", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--num_beams", type=int, default=1, help="beam search (greedy only; HF's semantics)")
    ap.add_argument("--num_return_sequences", type=int, default=1, help="beams returned per prompt, best first")
    ap.add_argument("--length_penalty", type=float, default=1.0)
    ap.add_argument("--early_stopping", action="store_true")
    ap.add_argument("--assistant_model", default=None,
                    help="a smaller model (name or directory) with the same vocabulary: greedy speculative decoding")
    ap.add_argument("--num_assistant_tokens", type=int, default=5, help="draft tokens per round (1..7)")
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--load_in_4bit", action="store_true",
                    help="keep the base model's linear layers in 4 bits (models/quant.py), as sft_llama2.py does")
    ap.add_argument("--bnb_4bit_quant_type", default="nf4", choices=("nf4", "fp4"))
    ap.add_argument("--device", default=None, help="cuda / cpu (default: cuda when there is one)")
    ap.add_argument("--config_overrides", default=None, help="e.g. n_layer=2,n_embd=128 for a named size")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    prompts = list(a.prompt)
    if a.prompt_file:
        with open(a.prompt_file) as f:
            prompts += [line.rstrip("\n") for line in f if line.strip()]
    if not prompts:
        raise SystemExit("generate.py: give --prompt or --prompt_file")
    device = torch.device(a.device or ("cuda" if torch.cuda.is_available() else "cpu"))
    config = load_config(a.model_name_or_path, a.config_overrides)
    model = build_model(config, a.model_name_or_path, torch_dtype="bfloat16" if a.bf16 else None)
    if a.load_in_4bit:
        # the QLoRA base of sft_llama2.py --load_in_4bit: every nn.Linear but the LM head in the 4-bit store,
        # quantised on the target device (the GPU kernel when there is one); adapters go on top
        from distributed_lion_pytorch_amd.models.quant import QuantConfig, quantize_model

        if a.bf16:
            model = model.to(torch.bfloat16)
        model = quantize_model(model.to(device), QuantConfig(bnb_4bit_quant_type=a.bnb_4bit_quant_type,
                                                             bnb_4bit_compute_dtype=torch.bfloat16 if a.bf16 else None))
    if a.adapter:
        model = load_adapter(model, a.adapter)
    if a.bf16:
        model = model.to(torch.bfloat16)
    model = model.to(device).eval()
    assistant = None
    if a.assistant_model:
        assistant = build_model(load_config(a.assistant_model), a.assistant_model, torch_dtype="bfloat16" if a.bf16 else None)
        if a.bf16:
            assistant = assistant.to(torch.bfloat16)
        assistant = assistant.to(device).eval()
    tok = load_tokenizer(a.model_name_or_path)

    rows = [tok.encode(p) or [getattr(tok, "bos_token_id", None) or 0] for p in prompts]
    vocab = model.config.vocab_size
    if max(max(r) for r in rows) >= vocab:
        raise SystemExit(f"generate.py: the tokenizer produces ids beyond the model's vocabulary ({vocab})")
    width = max(len(r) for r in rows)
    pad = getattr(tok, "pad_token_id", None)
    pad = pad if pad is not None and pad < vocab else 0
    ids = torch.full((len(rows), width), pad, dtype=torch.long)
    mask = torch.zeros(len(rows), width, dtype=torch.long)
    for b, r in enumerate(rows):  # left-padded, HF's generation convention
        ids[b, width - len(r):] = torch.tensor(r)
        mask[b, width - len(r):] = 1
    eos = getattr(tok, "eos_token_id", None)
    eos = eos if eos is not None and eos < vocab else None
    ids, mask = ids.to(device), mask.to(device)

    def sync():
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    sync()
    t0 = time.perf_counter()
    out = model.generate(ids, attention_mask=mask, max_new_tokens=a.max_new_tokens, do_sample=a.do_sample,
                         temperature=a.temperature, top_k=a.top_k, top_p=a.top_p, eos_token_id=eos,
                         pad_token_id=pad if eos is not None else None, seed=a.seed, num_beams=a.num_beams,
                         num_return_sequences=a.num_return_sequences, length_penalty=a.length_penalty,
                         early_stopping=a.early_stopping, assistant_model=assistant,
                         num_assistant_tokens=a.num_assistant_tokens, return_dict_in_generate=assistant is not None)
    sync()
    dt = time.perf_counter() - t0
    spec = None
    if assistant is not None:
        spec, out = out, out.sequences
    new = out[:, width:].tolist()
    n_tokens = 0
    per = a.num_return_sequences  # rows per prompt, best beam first
    for j, r in enumerate(new):
        p = prompts[j // per]
        if eos is not None and eos in r:
            r = r[:r.index(eos)]
        n_tokens += len(r)
        print(f"--- {p!r}{f' [beam {j % per}]' if per > 1 else ''}\n{tok.decode(r)}")
    print(f"[generate] {len(prompts)} prompt(s), {out.shape[1] - width} steps, {n_tokens} new tokens in {dt:.3f} s: "
          f"{n_tokens / dt:.1f} tokens/s on {device}")
    if spec is not None:
        print(f"[generate] speculative: {spec.rounds} rounds of up to {a.num_assistant_tokens} drafts, accepted per prompt "
              f"{spec.accepted.tolist()}")
    return out


if __name__ == "__main__":
    main()
