"""``predictions=True`` on the native causal-LM heads: evaluation without logits.

The head runs once through ops/fused.causal_lm_score (one GEMM, one read-only
kernel pass, csrc/lm_score.hip) and the output carries what the evaluation
loop reduces logits to anyway: one token and one rank per position."""
from dataclasses import dataclass
from typing import Optional

import torch
from transformers.utils import ModelOutput

from ..ops import fused


@dataclass
class ScoredCausalLMOutput(ModelOutput):
    """``predictions[:, t]`` is what ``logits[:, t].argmax(-1)`` would have been;
    ``label_ranks[:, t]`` is the rank of ``labels[:, t + 1]`` among the logits of
    position t (0: predicted; -1 where that label is -100 and at t = T - 1).
    ``logits`` is always None."""

    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    predictions: Optional[torch.Tensor] = None
    label_ranks: Optional[torch.Tensor] = None


def scored_output(model, h: torch.Tensor, weight: torch.Tensor, labels, normalizer=None) -> ScoredCausalLMOutput:
    """The ``predictions=True`` branch of a native model's forward: evaluation
    only, labels required; the module's label smoothing applies (z-loss is
    training-only, models/loss_options.py)."""
    if labels is None:
        raise ValueError("dlion: predictions=True needs labels (the rank is the label's)")
    if model.training:
        raise RuntimeError("dlion: predictions=True is an evaluation path (no gradient): call model.eval() first")
    with torch.no_grad():  # the op is forward-only and refuses to run where a gradient would be recorded
        s = fused.causal_lm_score(h, weight, labels, normalizer=normalizer, **model._loss_options())
    return ScoredCausalLMOutput(loss=s.loss, logits=None, predictions=s.pred, label_ranks=s.rank)
