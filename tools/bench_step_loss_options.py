"""One training step (TrainStep: micro-batches + clip + Lion) on the GPT-2 bench
config with label smoothing / z-loss, for the step-level A/B.

    python tools/bench_step_loss_options.py --mode fused --smoothing 0.1 [--z_loss 0] [--steps 6] [--out FILE]
    python tools/bench_step_loss_options.py --mode hf_smoother --smoothing 0.1

``fused``: the options go to the model (``set_loss_options``) and the loss is
computed by the fused LM-head cross-entropy.  ``hf_smoother``: what HF's
``Trainer.compute_loss`` does with ``--label_smoothing_factor`` on a model
without loss options -- the model is called without labels, returns the full
logits, and ``LabelSmoother`` computes the loss.  The second mode uses nothing
of this feature, so it also runs on a tree that predates it (the baseline).
Appends one line: tokens/s (median step) and the peak allocated memory."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.environ.get("DLION_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_lion_pytorch_amd import Lion  # noqa: E402
from distributed_lion_pytorch_amd.models.gpt2 import GPT2LMHeadModel, gpt2_config  # noqa: E402
from distributed_lion_pytorch_amd.trainer.engine import TrainStep  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["fused", "hf_smoother"], required=True)
    ap.add_argument("--smoothing", type=float, default=0.1)
    ap.add_argument("--z_loss", type=float, default=0.0)
    ap.add_argument("--model", default="gpt2")
    ap.add_argument("--micro_batch", type=int, default=20)
    ap.add_argument("--seq_len", type=int, default=1024)
    ap.add_argument("--grad_accum", type=int, default=8)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = gpt2_config(a.model, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0)
    model = GPT2LMHeadModel(cfg).to(device=dev, dtype=torch.bfloat16)
    opt = Lion(model.parameters(), lr=1e-4, weight_decay=0.1)
    if a.mode == "fused":
        model.set_loss_options(label_smoothing=a.smoothing, z_loss=a.z_loss)
        loss_fn = None
    else:
        from transformers.trainer_pt_utils import LabelSmoother

        if a.z_loss:
            raise SystemExit("HF's LabelSmoother has no z-loss")
        smoother = LabelSmoother(epsilon=a.smoothing)
        loss_fn = lambda m, b: smoother(m(b["input_ids"]), b["labels"], shift_labels=True)  # noqa: E731
    step = TrainStep(model, opt, grad_accum=a.grad_accum, max_grad_norm=1.0, loss_fn=loss_fn)
    gen = torch.Generator(device=dev).manual_seed(1)

    def batches():
        for _ in range(a.grad_accum):
            ids = torch.randint(0, cfg.vocab_size, (a.micro_batch, a.seq_len), device=dev, generator=gen)
            yield {"input_ids": ids, "labels": ids}

    times, loss = [], None
    for it in range(a.warmup + a.steps):
        mbs = list(batches())
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        loss = step(mbs)
        torch.cuda.synchronize(dev)
        if it >= a.warmup:
            times.append(time.perf_counter() - t0)
    times.sort()
    med = times[len(times) // 2]
    tokens = a.micro_batch * a.seq_len * a.grad_accum
    line = (f"{a.tag or a.mode:24s} smoothing {a.smoothing} z_loss {a.z_loss}: {tokens / med:10.0f} tokens/s "
            f"(median of {len(times)} steps, {med * 1e3:.1f} ms; min {times[0] * 1e3:.1f} max {times[-1] * 1e3:.1f}), "
            f"peak {torch.cuda.max_memory_allocated(dev) / 2 ** 30:.2f} GiB, last loss {loss.item():.4f}")
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
