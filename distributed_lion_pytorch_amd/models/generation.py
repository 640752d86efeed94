"""Generation for the native causal LMs: a token-major KV cache and ``generate``.

``KVCache`` holds, per layer, k / v buffers ``[B, max_len, Hkv, D]`` -- the layout the training path computes
k and v in, so the prefill writes them with plain copies -- and the per-row lengths on the device.  The models
take it as an optional ``cache`` argument (models/llama.py, models/gpt2.py): the first call is the prefill (the
prompt through the flash forward), every later call one decode step (one token per row through
``fused.kv_append`` and ``fused.decode_attention``, csrc/decode.hip) or a chunk of up to 8 tokens per row, ragged
by ``n_new`` (``fused.kv_append_chunk`` and ``fused.chunk_attention``, csrc/chunk_attention.hip), or with
``extend=True`` any number of tokens per row (``fused.extend_attention``, csrc/extend_attention.hip);
``KVCache.truncate`` rolls rows back.

``KVCache(..., kv_dtype="fp8_e4m3")`` (``generate(kv_cache_dtype="fp8_e4m3")``) holds e4m3 codes and one power-of-two
fp32 scale per (token, kv head) instead: (D + 4) / 2D of the bf16 cache's memory.  The prefill quantises the rotated
k and v with ``fused.kv_quantize`` (the prompt's own attention stays the flash forward on the unquantised k and v),
a step, a chunk or an ``extend=True`` forward of any length appends through the fp8 stores of ``fused.kv_append`` /
``kv_append_chunk`` and attends through ``fused.cached_attention_fp8`` (csrc/kv8_attention.hip up to 8 tokens per row,
csrc/kv8_extend_attention.hip above).  Only the cached keys and values are quantised; the tokens may differ from the
bf16 cache's.

``NativeGenerateMixin.generate`` uses HF's argument names: greedy or sampled (temperature, then top-k, then
top-p), ragged prompts by ``attention_mask`` (left- or right-padded), EOS / pad handling; ``num_beams > 1`` is beam
search (HF's semantics) on ``fused.lm_head_topk``; ``assistant_model`` is greedy speculative decoding (a draft
model proposes, one chunk forward of this model checks).  Out of scope: beam sampling, diverse / constrained
beams, repetition penalties, a paged or rolling cache (a windowed layer keeps its full-length cache and only
bounds the key range), graph capture.  ``sampler="speculative"`` with ``do_sample=True`` and an ``assistant_model`` is
speculative sampling: the assistant samples the drafts and ``fused.speculative_verify`` (csrc/spec_verify.hip) accepts
or resamples them, so the tokens are distributed as this model's own samples.
"""
from __future__ import annotations

import itertools
import random
from typing import NamedTuple, Optional

import torch

from ..ops import fused
from ..ops.linear import gemm_fwd

_EOS_CHECK_EVERY = 8  # decode steps between two host reads of "every row has finished"
KV_CACHE_DTYPES = (None, "fp8_e4m3")  # None: the model's dtype
BEAM_CACHES = ("repeated", "shared")  # beam search: a private copy of the prompt's cache per beam, or one per prompt


class GenerateOutput(NamedTuple):
    """``generate(..., return_dict_in_generate=True)``: ``sequences`` [rows, T0 + n_new] and, for beam search,
    ``sequences_scores`` [rows]: the sum of the new tokens' log-probabilities / (their number ** length_penalty)."""

    sequences: torch.Tensor
    sequences_scores: Optional[torch.Tensor]


class SpeculativeOutput(NamedTuple):
    """``generate(..., assistant_model=m, return_dict_in_generate=True)``: ``sequences`` as without an assistant,
    ``rounds`` (int: draft + verify rounds run) and ``accepted`` [rows]: the draft tokens each row accepted."""

    sequences: torch.Tensor
    sequences_scores: Optional[torch.Tensor]
    rounds: int
    accepted: torch.Tensor


def cache_geometry(config):
    """(layers, kv heads, head_dim) of a GPT-2 or Llama-family config."""
    if getattr(config, "model_type", "") == "gpt2":
        return config.n_layer, config.n_head, config.n_embd // config.n_head
    hd = getattr(config, "head_dim", None) or config.hidden_size // config.num_attention_heads
    return config.num_hidden_layers, config.num_key_value_heads, hd


class KVCache:
    """Per-layer key / value buffers [B, max_len, Hkv, D] and the rows' lengths (int32, on the device).
    Allocated once per ``generate`` call.  ``width`` is the host's bound on the lengths (prompt width plus
    steps taken): it sizes the decode grid and refuses a step past ``max_len`` without a device sync."""

    def __init__(self, config, batch: int, max_len: int, device=None, dtype=torch.float32, kv_dtype=None):
        layers, hkv, hd = cache_geometry(config)
        self.batch, self.max_len = int(batch), int(max_len)
        if self.batch < 1 or self.max_len < 1:
            raise ValueError("KVCache: batch and max_len must be positive")
        if kv_dtype not in KV_CACHE_DTYPES:
            raise ValueError(f"KVCache: kv_dtype must be one of {KV_CACHE_DTYPES}, got {kv_dtype!r}")
        self.kv_dtype = kv_dtype
        # one allocation: [layer, k | v, B, max_len, Hkv, D]; "fp8_e4m3": e4m3 codes (uint8) and one fp32 scale per
        # (token, kv head) in a second one (ops/fused.py kv_quantize_reference has the format)
        self._buf = torch.zeros(layers, 2, self.batch, self.max_len, hkv, hd, device=device,
                                dtype=dtype if kv_dtype is None else torch.uint8)
        self._scales = None if kv_dtype is None else torch.zeros(layers, 2, self.batch, self.max_len, hkv, device=device)
        self.lengths = torch.zeros(self.batch, dtype=torch.int32, device=device)
        self.kv_len = self.lengths  # lengths + 1 during a decode step
        self.width = 0
        self.prefilled = False
        self.chunk = False  # the forward in flight takes the chunk path (T > 1 tokens per row, or ragged)
        self.n_new = None  # int32 [B]: the tokens of the chunk in flight that row b keeps (None: all T)

    def layer(self, i: int):
        """(k, v) of layer i, each [B, max_len, Hkv, D] (an fp8 cache: the codes)."""
        return self._buf[i, 0], self._buf[i, 1]

    def layer_scales(self, i: int):
        """(k scales, v scales) of layer i of an fp8 cache, each fp32 [B, max_len, Hkv]; (None, None) otherwise."""
        if self._scales is None:
            return None, None
        return self._scales[i, 0], self._scales[i, 1]

    def begin(self, B: int, T: int, n_new: Optional[torch.Tensor] = None, extend: bool = False) -> bool:
        """Start a forward of T tokens per row; True for the prefill (the first call).  After the prefill T = 1
        is a decode step and 1 < T <= 8 a chunk (``fused.kv_append_chunk`` / ``fused.chunk_attention``), of
        which row b keeps the first ``n_new[b]`` tokens ([B], 0 <= n_new[b] <= T; None: all T).  ``extend``
        accepts any T >= 1 that fits (``fused.extend_attention``: a new turn, a prompt prefilled in pieces)."""
        if B != self.batch:
            raise ValueError(f"KVCache: built for batch {self.batch}, got {B}")
        if torch.is_grad_enabled():
            raise RuntimeError("KVCache: the cached forward is inference only; call it under torch.no_grad()")
        if not self.prefilled:
            if n_new is not None:
                raise ValueError("KVCache: n_new belongs to a chunk after the prefill (ragged prompts: set_lengths)")
            if T > self.max_len:
                raise ValueError(f"KVCache: a prompt of {T} tokens does not fit max_len {self.max_len}")
            return True
        if T < 1 or (T > fused.CHUNK_MAX_TOKENS and not extend):
            raise ValueError(f"KVCache: after the prefill a forward takes 1 to {fused.CHUNK_MAX_TOKENS} tokens per row"
                             " (more with extend=True)")
        if self.width + T > self.max_len:
            raise ValueError(f"KVCache: full ({self.max_len} positions)")
        self.chunk = T > 1 or n_new is not None
        if self.chunk:
            if n_new is not None and tuple(n_new.shape) != (B,):
                raise ValueError("KVCache: n_new must be [B]")
            self.n_new = None if n_new is None else n_new.to(device=self.lengths.device, dtype=torch.int32)
            self.kv_len = self.lengths  # the chunk ops take the lengths before the chunk
        else:
            self.kv_len = self.lengths + 1
        return False

    def advance(self, T: int) -> None:
        if not self.prefilled:
            self.lengths.fill_(T)
            self.width, self.prefilled = T, True
        elif self.chunk:
            if self.n_new is None:
                self.lengths += T
            else:
                self.lengths += self.n_new.clamp(0, T)
            self.width += T
            self.chunk, self.n_new = False, None
        else:
            self.lengths += 1
            self.width += 1

    def truncate(self, lengths: torch.Tensor, width: int) -> None:
        """Roll rows back (speculative decoding: rejected drafts): row b now holds ``lengths[b]`` tokens, not more
        than it did, and ``width`` is the caller's host bound on them.  No data moves: nothing at or beyond a
        row's length is ever read, and the next forward overwrites it."""
        width = int(width)
        if not self.prefilled or not 0 <= width <= self.width:
            raise ValueError(f"KVCache.truncate: width must be in [0, {self.width}] of a prefilled cache")
        self.lengths.copy_(lengths.to(self.lengths.dtype))
        self.kv_len = self.lengths
        self.width = width

    def set_lengths(self, lengths: torch.Tensor) -> None:
        """Ragged prompts, left-aligned in the prefill: row b holds ``lengths[b]`` <= width real tokens."""
        self.lengths.copy_(lengths.to(self.lengths.dtype))

    def repeat_rows(self, n: int) -> "KVCache":
        """A new cache of batch ``batch * n`` whose rows b n .. b n + n - 1 hold row b (beam search after one
        prefill per prompt): only the positions below ``width`` are copied, the lengths are repeated."""
        n = int(n)
        if n < 1:
            raise ValueError("KVCache.repeat_rows: n must be >= 1")
        out = object.__new__(KVCache)
        out.batch, out.max_len, out.kv_dtype = self.batch * n, self.max_len, self.kv_dtype
        w = self.width

        def repeated(buf):
            if buf is None:
                return None
            shape = list(buf.shape)
            shape[2] = out.batch
            new = torch.zeros(shape, device=buf.device, dtype=buf.dtype)
            new[:, :, :, :w] = buf[:, :, :, :w].repeat_interleave(n, dim=2)
            return new

        out._buf, out._scales = repeated(self._buf), repeated(self._scales)
        out.lengths = self.lengths.repeat_interleave(n)
        out.kv_len = out.lengths
        out.width, out.prefilled = self.width, self.prefilled
        out.chunk, out.n_new = False, None
        return out

    def reorder_rows(self, index: torch.Tensor, lo: int = 0) -> None:
        """Row r takes the contents of row ``index[r]`` (beam search: the beam it continues) at the positions
        ``lo <= t < width``, and its length.  Below ``lo`` the caller vouches that the rows exchanged hold the
        same keys (a shared prompt), so the move costs the generated suffix, not the context."""
        lo = max(0, int(lo))
        if lo < self.width:
            for buf in (self._buf,) if self._scales is None else (self._buf, self._scales):
                buf[:, :, :, lo:self.width] = buf[:, :, :, lo:self.width].index_select(2, index)
        self.lengths.copy_(self.lengths.index_select(0, index))


class BeamKVCache:
    """Beam search on a shared prompt cache: ``prefix``, the prefilled ``KVCache`` of the B prompts exactly as the
    prefill left it (its width is the prompt's, no room for new tokens), and ``suffix``, a ``KVCache`` of ``B * beams``
    rows and ``max_new_tokens`` positions for what the beams generate.  Beam row ``r = b * beams + j`` attends prompt
    b's prefix keys and its own suffix keys (``fused.kv_append_suffix`` / ``fused.shared_prefix_attention``,
    csrc/prefix_attention.hip): no prompt key is copied.  The models drive it through ``begin`` / ``advance`` like a
    ``KVCache``, for single-token steps only."""

    def __init__(self, prefix: KVCache, beams: int, max_new_tokens: int, config, dtype=torch.float32):
        if not prefix.prefilled or prefix.kv_dtype is not None:
            raise ValueError("BeamKVCache: the prefix must be a prefilled cache in the model's dtype")
        self.prefix, self.beams = prefix, int(beams)
        if self.beams < 2:
            raise ValueError("BeamKVCache: beams must be >= 2")
        self.batch = prefix.batch * self.beams
        dev = prefix.lengths.device
        self.suffix = KVCache(config, self.batch, max_new_tokens, dev, dtype)
        self.suffix.prefilled = True  # empty rows that take single-token steps
        self.max_len = prefix.max_len + self.suffix.max_len  # the positions a rotary table must cover
        self.prefix_len = prefix.lengths  # int32 [B]
        self._base = prefix.lengths.repeat_interleave(self.beams)
        self.positions = self._base  # int32 [B * beams]: the total position of the token of the step in flight

    def begin(self, B: int, T: int, n_new: Optional[torch.Tensor] = None, extend: bool = False) -> bool:
        """Start a decode step of one token per beam row; never the prefill (always False)."""
        if T != 1 or n_new is not None or extend:
            raise ValueError("BeamKVCache: a forward takes one token per beam row (no chunks, no extend)")
        self.suffix.begin(B, 1)
        self.positions = self._base + self.suffix.lengths
        return False

    def advance(self, T: int) -> None:
        self.suffix.advance(T)

    def reorder_rows(self, index: torch.Tensor) -> None:
        """Beam row r continues beam ``index[r]`` of the same prompt: only the suffix moves."""
        self.suffix.reorder_rows(index)


# ------------------------------------------------------------------------------------------ prompts
def left_align(input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor]):
    """(ids with every row's tokens moved to the left edge, lengths [B]); the mask may be left- or right-padded
    but must be one contiguous run of ones per row."""
    B, T = input_ids.shape
    if attention_mask is None:
        return input_ids, torch.full((B,), T, dtype=torch.long, device=input_ids.device)
    if attention_mask.shape != input_ids.shape:
        raise ValueError("generate: attention_mask must have the shape of input_ids")
    m = attention_mask.to(input_ids.device) != 0
    n = m.sum(1)
    start = m.to(torch.int8).argmax(1)
    idx = torch.arange(T, device=input_ids.device)[None, :]
    run = (idx >= start[:, None]) & (idx < (start + n)[:, None])
    if bool((n == 0).any()) or not bool((run == m).all()):
        raise ValueError("generate: attention_mask needs one contiguous, non-empty run of ones per row "
                         "(left- or right-padded prompts)")
    ids = input_ids.gather(1, (idx + start[:, None]).clamp_max(T - 1))
    return torch.where(idx < n[:, None], ids, torch.zeros_like(ids)), n


# ------------------------------------------------------------------------------------------ sampling
def warp_logits(logits: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
    """fp32 logits [B, V] after temperature, then top-k, then top-p (HF's order and definitions: top-p keeps the
    smallest set of most likely tokens whose probability reaches top_p); removed tokens are -inf."""
    logits = logits.float()
    if temperature != 1.0:
        logits = logits / float(temperature)
    if top_k and 0 < int(top_k) < logits.shape[-1]:
        kth = torch.topk(logits, int(top_k), dim=-1).values[:, -1:]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    if top_p < 1.0:
        srt, order = torch.sort(logits, dim=-1, descending=False)
        remove = srt.softmax(-1).cumsum(-1) <= (1.0 - float(top_p))
        remove[:, -1] = False
        logits = logits.masked_fill(torch.zeros_like(remove).scatter(1, order, remove), float("-inf"))
    return logits


class NativeGenerateMixin:
    """``generate`` for GPT2LMHeadModel and LlamaForCausalLM (Mistral, Qwen2 and Qwen3 inherit it).

    Not named ``...GenerationMixin``: transformers' ``PreTrainedModel.can_generate`` looks for that substring in
    the base classes and would then attach a ``generation_config`` and write ``generation_config.json`` on save;
    checkpoints stay what they were."""

    def _decoder(self):
        return self.transformer if hasattr(self, "transformer") else self.model

    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                 max_new_tokens: int = 20, do_sample: bool = False, temperature: float = 1.0, top_k: int = 0,
                 top_p: float = 1.0, eos_token_id=None, pad_token_id: Optional[int] = None,
                 seed: Optional[int] = None, num_beams: int = 1, num_return_sequences: int = 1,
                 length_penalty: float = 1.0, early_stopping: bool = False, return_dict_in_generate: bool = False,
                 assistant_model=None, num_assistant_tokens: int = 5, kv_cache_dtype: Optional[str] = None,
                 prefill_chunk_size: Optional[int] = None, sampler: str = "torch", beam_cache: str = "repeated"):
        """[B, T0] prompts -> [B, T0 + n_new] long: the prompt exactly as given, then the new tokens.

        Greedy takes the top-1 of ``fused.lm_head_score`` (the lowest id on ties, no [B, V] tensor); sampling
        warps the last hidden states' logits (temperature, top-k, top-p) and draws with ``torch.multinomial``
        from a generator seeded by ``seed``.  Rows that emitted ``eos_token_id`` (int or list) produce
        ``pad_token_id`` (default: the first EOS id) from then on; generation ends once every row has finished
        (read from the device every 8 steps; the result is trimmed to the step at which the last row finished).

        ``num_beams > 1`` is beam search with the semantics of transformers' ``generate(num_beams=n,
        do_sample=False)``: ``num_return_sequences`` rows per prompt, best first ([B * num_return_sequences,
        T0 + n_new]), ``length_penalty`` and ``early_stopping`` (False or True) as there; every step takes the
        ``max(2, 1 + #eos) * num_beams`` best continuations of every live beam from ``fused.lm_head_topk``.
        ``return_dict_in_generate=True`` returns :class:`GenerateOutput` (``sequences``, ``sequences_scores``; the
        scores are None without beams).

        ``assistant_model`` (a native causal LM with the same vocabulary size) turns greedy decoding into greedy
        speculative decoding: per round the assistant drafts up to ``num_assistant_tokens`` (1..7) tokens with
        single-token steps and this model checks them in one chunk forward (``fused.chunk_attention``), keeping
        the longest prefix it agrees with plus its own next token -- the tokens plain greedy decoding produces,
        for fewer passes over this model's weights.  ``return_dict_in_generate=True`` then returns
        :class:`SpeculativeOutput`.

        ``kv_cache_dtype="fp8_e4m3"`` keeps the cached keys and values as e4m3 codes with one power-of-two fp32 scale
        per (token, kv head) (``fused.kv_quantize``, the fp8 stores of ``fused.kv_append`` / ``kv_append_chunk``,
        ``fused.cached_attention_fp8``): the cache takes (D + 4) / 2D of the bf16 cache's memory (0.52 at head_dim
        128, 0.53 at 64).  Only what is cached is quantised -- the prompt's own attention in the prefill runs on the
        unquantised k and v, q and the probabilities stay bf16 / fp32 -- so the tokens may differ from the bf16
        cache's wherever two logits are closer than the quantisation error.  With ``assistant_model`` this model's
        cache takes the type and the assistant's stays in its own dtype.  Default None: the model's dtype.

        ``prefill_chunk_size=N`` prefills the prompt in pieces, which bounds the prefill's activation memory by N
        columns: the flash forward of the first N columns, then forwards of N columns each on the cache
        (``extend=True``: ``fused.kv_append_chunk`` and ``fused.extend_attention``), ragged prompts by ``n_new``; every
        row's last hidden state is taken from the piece it falls in.  It applies to greedy decoding, sampling, beam
        search and the target of ``assistant_model``.  Default None: one prefill of the whole prompt.

        ``sampler="fused"`` (with ``do_sample=True``) takes step i's tokens from ``fused.lm_head_sample(h, weight,
        temperature, top_k, top_p, seed, step=i)``: the head GEMM and one kernel launch (csrc/lm_sample.hip), no
        [B, V] fp32 tensor and no ``torch.Generator``.  The draw is Gumbel-max on a hash of (seed, step, row, token),
        so a seed gives other tokens than it gives under ``"torch"`` (the default: the warp / softmax / multinomial
        chain), and top-p keeps or drops equal logits together; ``seed=None`` takes one random seed per call.

        ``sampler="speculative"`` (with ``do_sample=True`` and an ``assistant_model``) is speculative sampling: per
        round the assistant samples up to ``num_assistant_tokens`` drafts from its own filtered distribution q
        (``fused.lm_sample``, the same temperature, top-k and top-p), this model scores them in one chunk forward,
        and ``fused.speculative_verify`` (csrc/spec_verify.hip) keeps draft x with probability min(1, p(x) / q(x)),
        replaces the first one it drops by a draw from norm(max(0, p - q)) and adds a draw from p when none is
        dropped.  The tokens are distributed as ``sampler="fused"``'s, whatever the assistant is; they are not the
        same tokens for a seed.  Both heads' logits must have one dtype for the kernel (else the PyTorch form runs).
        Returns :class:`SpeculativeOutput` as the greedy path does.

        ``beam_cache="shared"`` (with ``num_beams > 1``) keeps the prompt's keys and values once per prompt instead
        of once per beam: a :class:`BeamKVCache` of the prefill's cache (allocated at the prompt's width) and a suffix
        cache of ``B * num_beams`` rows for the generated tokens; every step runs ``fused.kv_append_suffix`` and
        ``fused.shared_prefix_attention`` (csrc/prefix_attention.hip), whose prefix blocks stream a prompt's keys once
        for all its beams.  The cache takes ``T0 + num_beams * max_new_tokens`` positions per prompt instead of
        ``num_beams * (T0 + max_new_tokens)``.  The same search; the scores differ from the default's by rounding.
        It needs the model's dtype for the cache and ``num_beams * H / Hkv <= 64``.  Default ``"repeated"``: one
        private copy of the prompt's cache per beam (``KVCache.repeat_rows``)."""
        if beam_cache not in BEAM_CACHES:
            raise ValueError(f"generate: beam_cache must be one of {BEAM_CACHES}, got {beam_cache!r}")
        if sampler not in ("torch", "fused", "speculative"):
            raise ValueError(f"generate: sampler must be 'torch', 'fused' or 'speculative', got {sampler!r}")
        if sampler == "speculative" and (not do_sample or num_beams != 1 or assistant_model is None):
            raise ValueError("generate: sampler='speculative' is speculative sampling; it needs do_sample=True, an "
                             "assistant_model and num_beams=1")
        if sampler == "fused" and (not do_sample or num_beams != 1 or assistant_model is not None):
            raise ValueError("generate: sampler='fused' is the sampling kernel; it needs do_sample=True, num_beams=1 "
                             "and no assistant_model")
        if prefill_chunk_size is not None:
            prefill_chunk_size = int(prefill_chunk_size)
            if prefill_chunk_size < 1:
                raise ValueError(f"generate: prefill_chunk_size must be >= 1, got {prefill_chunk_size}")
        if kv_cache_dtype not in KV_CACHE_DTYPES:
            raise ValueError(f"generate: kv_cache_dtype must be one of {KV_CACHE_DTYPES}, got {kv_cache_dtype!r}")
        num_beams, num_return_sequences = int(num_beams), int(num_return_sequences)
        if num_beams < 1:
            raise ValueError("generate: num_beams must be >= 1")
        if num_return_sequences < 1 or num_return_sequences > num_beams:
            raise ValueError("generate: num_return_sequences must be in [1, num_beams]"
                             + (" (more than one sequence per prompt needs num_beams > 1)" if num_beams == 1 else ""))
        if num_beams > 1 and do_sample:
            raise ValueError("generate: num_beams > 1 with do_sample=True (beam sampling) is not supported")
        if beam_cache == "shared":
            if num_beams == 1:
                raise ValueError("generate: beam_cache='shared' shares a prompt's cache among beams; it needs num_beams > 1")
            if kv_cache_dtype is not None:
                raise ValueError(f"generate: beam_cache='shared' keeps the cache in the model's dtype; kv_cache_dtype="
                                 f"{kv_cache_dtype!r} is not supported with it")
            group = cache_geometry(self.config)
            heads = self.config.n_head if self.config.model_type == "gpt2" else self.config.num_attention_heads
            if num_beams * (heads // group[1]) > fused.PREFIX_MAX_ROWS:
                raise ValueError(f"generate: beam_cache='shared' serves num_beams * H / Hkv <= {fused.PREFIX_MAX_ROWS} "
                                 f"query rows per prompt and kv head, got {num_beams} * {heads // group[1]}")
        if not isinstance(early_stopping, bool):
            raise ValueError(f"generate: early_stopping must be False or True, got {early_stopping!r}")
        if self.training:
            raise ValueError("generate: the model is in training mode; call model.eval() first")
        if input_ids.dim() != 2 or input_ids.shape[1] < 1:
            raise ValueError("generate: input_ids must be [B, T0] with T0 >= 1")
        max_new_tokens = int(max_new_tokens)
        if max_new_tokens < 1:
            raise ValueError("generate: max_new_tokens must be >= 1")
        if do_sample and not temperature > 0:
            raise ValueError("generate: temperature must be > 0")
        if do_sample and not 0.0 < top_p <= 1.0:
            raise ValueError("generate: top_p must be in (0, 1]")
        B, T0 = input_ids.shape
        total = T0 + max_new_tokens
        cfg = self.config
        if cfg.model_type == "gpt2" and total > cfg.n_positions:
            raise ValueError(f"generate: {T0} prompt + {max_new_tokens} new tokens exceed GPT-2's {cfg.n_positions} "
                             "learned positions (max_position_embeddings)")
        dev = input_ids.device
        eos = None
        if eos_token_id is not None:
            eos = torch.as_tensor([eos_token_id] if isinstance(eos_token_id, int) else list(eos_token_id), device=dev)
            if pad_token_id is None:
                pad_token_id = int(eos[0])
        if assistant_model is not None:
            if (do_sample and sampler != "speculative") or num_beams != 1:
                raise ValueError("generate: assistant_model is greedy speculative decoding; it needs do_sample=False "
                                 "and num_beams=1 (speculative sampling and assisted beam search are not supported)")
            k = int(num_assistant_tokens)
            if not 1 <= k <= fused.CHUNK_MAX_TOKENS - 1:
                raise ValueError(f"generate: num_assistant_tokens must be in [1, {fused.CHUNK_MAX_TOKENS - 1}] (the "
                                 f"target checks the drafts and one more token in a chunk of at most "
                                 f"{fused.CHUNK_MAX_TOKENS}), got {num_assistant_tokens}")
            acfg = assistant_model.config
            if acfg.vocab_size != cfg.vocab_size:
                raise ValueError(f"generate: the assistant's vocabulary ({acfg.vocab_size}) differs from the "
                                 f"model's ({cfg.vocab_size})")
            if assistant_model.training:
                raise ValueError("generate: the assistant model is in training mode; call assistant_model.eval() first")
            if acfg.model_type == "gpt2" and total > acfg.n_positions:
                raise ValueError(f"generate: {T0} prompt + {max_new_tokens} new tokens exceed the assistant's "
                                 f"{acfg.n_positions} learned positions")
        ids, lens = left_align(input_ids, attention_mask)
        weight = self.lm_head.weight
        if assistant_model is not None:
            sampling = None
            if sampler == "speculative":
                sampling = (float(temperature), int(top_k), float(top_p),
                            int(seed) if seed is not None else random.getrandbits(63), itertools.count())
            out = self._speculative(assistant_model, input_ids, ids, lens, max_new_tokens, eos, pad_token_id, k,
                                    kv_cache_dtype, prefill_chunk_size, sampling)
            fused.check_index_errors()
            return out if return_dict_in_generate else out.sequences
        if num_beams > 1:
            lo = T0 if attention_mask is None else int(lens.min())
            out = self._beam_search(input_ids, ids, lens, lo, max_new_tokens, eos, pad_token_id, num_beams,
                                    num_return_sequences, float(length_penalty), early_stopping, kv_cache_dtype,
                                    prefill_chunk_size, beam_cache == "shared")
            fused.check_index_errors()
            return out if return_dict_in_generate else out.sequences
        cache = KVCache(cfg, B, total, dev, weight.dtype, kv_cache_dtype)
        gen = None
        if sampler == "fused":
            draw_seed = int(seed) if seed is not None else random.getrandbits(63)
        elif do_sample and seed is not None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed))

        base = self._decoder()
        h = self._prefill(base, ids, lens, cache, prefill_chunk_size)
        new = torch.empty(B, max_new_tokens, dtype=torch.long, device=dev)
        finished = torch.zeros(B, dtype=torch.bool, device=dev)
        done_at = torch.full((B,), max_new_tokens, dtype=torch.long, device=dev)  # the step a row emitted EOS at
        ignore = torch.full((B,), -100, dtype=torch.long, device=dev)
        for i in range(max_new_tokens):
            if sampler == "fused":
                tok = fused.lm_head_sample(h, weight, temperature, top_k, top_p, draw_seed, step=i).ids.long()
            elif do_sample:
                logits = warp_logits(gemm_fwd(h, weight), temperature, top_k, top_p)
                tok = torch.multinomial(logits.softmax(-1), 1, generator=gen)[:, 0]
            else:
                tok = fused.lm_head_score(h, weight, ignore).pred.long()
            if eos is not None:
                tok = torch.where(finished, torch.full_like(tok, pad_token_id), tok)
                hit = torch.isin(tok, eos) & ~finished
                done_at = torch.where(hit, torch.full_like(done_at, i), done_at)
                finished = finished | hit
            new[:, i] = tok
            if i + 1 == max_new_tokens:
                break
            if eos is not None and (i + 1) % _EOS_CHECK_EVERY == 0 and bool(finished.all()):
                break
            h = base(tok[:, None], cache=cache)[:, 0]
        n_new = i + 1
        if eos is not None:
            last = int(done_at.max())  # the one read at the end: the step the last row finished at
            if last < max_new_tokens:
                n_new = last + 1
        fused.check_index_errors()
        out = torch.cat([input_ids, new[:, :n_new]], dim=1)
        return GenerateOutput(out, None) if return_dict_in_generate else out

    @staticmethod
    def _prefill(base, ids, lens, cache, piece=None):
        """The prompt into a fresh cache: the hidden state [B, C] of every row's last real token, the cache's lengths
        set to ``lens``.  ``piece`` (generate's ``prefill_chunk_size``): the flash forward of the first ``piece``
        columns, then extend forwards of ``piece`` columns each, of which row b keeps ``clamp(lens[b] - offset, 0,
        piece)``; None, or a prompt no wider than ``piece``: one forward of the whole prompt."""
        B, T0 = ids.shape
        rows = torch.arange(B, device=ids.device)
        if piece is None or piece >= T0:
            h = base(ids, cache=cache)[rows, lens - 1]
            cache.set_lengths(lens)
            return h
        last = lens - 1
        h = base(ids[:, :piece], cache=cache)[rows, last.clamp_max(piece - 1)]
        cache.set_lengths(lens.clamp_max(piece))
        for off in range(piece, T0, piece):
            cols = ids[:, off:off + piece]
            w = cols.shape[1]
            hp = base(cols, cache=cache, n_new=(lens - off).clamp(0, w).to(torch.int32), extend=True)
            here = (last >= off) & (last < off + w)
            h = torch.where(here[:, None], hp[rows, (last - off).clamp(0, w - 1)], h)
        return h

    def _speculative(self, assistant, input_ids, ids, lens, n, eos, pad_token_id, k, kv_cache_dtype=None,
                     prefill_chunk_size=None, sampling=None):
        """Speculative decoding: greedy, or with ``sampling`` (temperature, top_k, top_p, seed, step counter)
        speculative sampling, which differs in how a token is chosen and a draft judged (``_speculative_sample``)
        and in nothing of the bookkeeping below.  Row b has emitted ``count[b]`` tokens, the last of which (``last``) is not
        in the target's cache yet; the assistant's cache lacks the last one or two of them (``unseen``: two when
        every draft of the previous round was accepted, since the last draft was never fed to the assistant).  A
        round: the assistant absorbs ``unseen`` in a ragged chunk of 2 and drafts kk tokens (kk - 1 single-token
        steps), the target runs one chunk of ``last`` and the drafts, row b keeps the ``a[b]`` drafts that equal the
        target's top-1 (sampling: that pass the accept test) and the target's next token, and both caches are rolled back to what stays valid.  Rows
        that have emitted EOS or all n tokens are parked at length 0 (their forwards go on, unread).  One host
        read per round: whether a row is still open, and the caches' widths."""
        B, T0 = input_ids.shape
        dev = input_ids.device
        cfg, weight, base = self.config, self.lm_head.weight, self._decoder()
        acfg, a_weight, a_base = assistant.config, assistant.lm_head.weight, assistant._decoder()
        size = T0 + n + k + 1  # the last round may run k + 1 positions past the last kept token
        limit_t = min(size, cfg.n_positions) if cfg.model_type == "gpt2" else size
        limit_a = min(size, acfg.n_positions) if acfg.model_type == "gpt2" else size
        rows = torch.arange(B, device=dev)
        cache = KVCache(cfg, B, size, dev, weight.dtype, kv_cache_dtype)
        a_cache = KVCache(acfg, B, size, dev, a_weight.dtype)
        h = self._prefill(base, ids, lens, cache, prefill_chunk_size)
        a_base(ids, cache=a_cache)
        a_cache.set_lengths(lens)

        def top1(hidden, w):
            flat = hidden.reshape(-1, hidden.shape[-1])
            return fused.lm_head_score(flat, w, torch.full((flat.shape[0],), -100, dtype=torch.long, device=dev)).pred.long()

        new = torch.zeros(B, n + k + 1, dtype=torch.long, device=dev)
        if sampling is None:
            last = top1(h, weight)
        else:
            temperature, top_k, top_p, seed, steps = sampling
            last = fused.lm_head_sample(h, weight, temperature, top_k, top_p, seed, next(steps)).ids.long()
        new[:, 0] = last
        count = torch.ones(B, dtype=torch.long, device=dev)
        accepted = torch.zeros(B, dtype=torch.long, device=dev)
        finished = torch.isin(last, eos) if eos is not None else torch.zeros(B, dtype=torch.bool, device=dev)
        active = ~finished & (count < n)
        t_len, a_len = lens.clone(), lens.clone()  # the caches' lengths (long)
        unseen = torch.stack([last, last], dim=1)
        n_unseen = torch.ones(B, dtype=torch.long, device=dev)
        rounds = 0
        t_width = a_width = T0
        go_on = n > 1 and bool(active.any())
        if go_on and not bool(active.all()):
            t_len, a_len, n_unseen = t_len * active, a_len * active, n_unseen * active
            cache.truncate(t_len, t_width)
            a_cache.truncate(a_len, a_width)
        while go_on:
            kk = min(k, limit_t - t_width - 1, limit_a - a_width - 1)  # >= 1: an open row has room for 2 more tokens
            rounds += 1
            # the assistant: absorb the accepted tokens it has not seen, then draft
            ha = a_base(unseen, cache=a_cache, n_new=n_unseen.to(torch.int32))
            ha = ha[rows, (n_unseen - 1).clamp_min(0)]
            if sampling is None:
                drafts = [top1(ha, a_weight)]
                for _ in range(kk - 1):
                    drafts.append(top1(a_base(drafts[-1][:, None], cache=a_cache)[:, 0], a_weight))
                drafts = torch.stack(drafts, dim=1)  # [B, kk]
                # the target: one chunk over the last emitted token and the drafts
                chunk = torch.cat([last[:, None], drafts], dim=1)
                pred = top1(base(chunk, cache=cache), weight).view(B, kk + 1)  # the target's token after each of the chunk's inputs
                a = (pred[:, :kk] == drafts).long().cumprod(1).sum(1)  # accepted drafts
            else:
                drafts, pred, a = self._speculative_sample(sampling, ha, lambda t: a_base(t[:, None], cache=a_cache)[:, 0],
                                                           a_weight, last, lambda c: base(c, cache=cache), weight, kk)
            adv = torch.where(active, torch.minimum(a + 1, n - count), torch.zeros_like(a))
            step = torch.arange(kk + 1, device=dev)
            keep = step[None, :] < adv[:, None]
            at = (count[:, None] + step[None, :]).clamp_max(new.shape[1] - 1)
            new.scatter_(1, at, torch.where(keep, pred, new.gather(1, at)))
            if eos is not None:
                finished = finished | (keep & torch.isin(pred, eos)).any(1)
            accepted += torch.minimum(a, adv)
            count = count + adv
            last = torch.where(adv > 0, pred.gather(1, (adv - 1).clamp_min(0)[:, None])[:, 0], last)
            active = active & ~finished & (count < n)
            # roll back: the target keeps `last` and the accepted drafts, the assistant what it was fed of them
            full = adv == kk + 1
            fed = torch.minimum(adv - 1, torch.full_like(adv, kk - 1)).clamp_min(0)
            t_len = (t_len + adv) * active
            a_len = (a_len + n_unseen + fed) * active
            n_unseen = torch.where(full, 2, 1) * active
            unseen = torch.stack([torch.where(full, drafts[:, kk - 1], last), last], dim=1)
            state = torch.stack([active.any().long(), t_len.max(), a_len.max()]).tolist()  # the round's host read
            go_on, t_width, a_width = bool(state[0]), int(state[1]), int(state[2])
            cache.truncate(t_len, t_width)
            a_cache.truncate(a_len, a_width)
        n_out = n
        new = new[:, :n]
        if eos is not None:
            step = torch.arange(n, device=dev)
            first = torch.where(torch.isin(new, eos), step[None, :], torch.full_like(new, n)).min(1).values
            new = torch.where(step[None, :] > first[:, None], torch.full_like(new, pad_token_id), new)
            done = int(first.max())
            if done < n:
                n_out = done + 1
        out = torch.cat([input_ids, new[:, :n_out]], dim=1)
        return SpeculativeOutput(out, None, rounds, accepted)

    @staticmethod
    def _speculative_sample(sampling, ha, a_step, a_weight, last, t_chunk, weight, kk):
        """One round's drafts and verdict under sampling: (drafts [B, kk], emitted [B, kk + 1], accepted [B]), row b
        emitting ``drafts[b, :accepted[b]]`` and then the verify's ``next[b]``.  ``ha`` [B, C] is the assistant's
        hidden state after the last emitted token, ``a_step(tokens)`` its single-token cached step and
        ``t_chunk(tokens)`` the target's chunk forward.  Every draft step keeps its head's logits and the sampler's
        floor; the target's ``kk + 1`` rows go through one ``fused.lm_sample`` (their floors, and the bonus token at
        position kk), then ``fused.speculative_verify``.  Each launch takes the next value of the call's step
        counter, so the drafts' noise, the target's, the accept uniforms and the residual's are independent."""
        temperature, top_k, top_p, seed, steps = sampling
        v = weight.shape[0]
        drafts, d_logits, d_floor = [], [], []
        for j in range(kk):
            if j:
                ha = a_step(drafts[-1])
            d_logits.append(fused.lm_head_logits(ha, a_weight))
            drawn = fused.lm_sample(d_logits[-1], v, temperature, top_k, top_p, seed, next(steps))
            drafts.append(drawn.ids.long())
            d_floor.append(drawn.floor)
        drafts = torch.stack(drafts, dim=1)
        B = drafts.shape[0]
        t_logits = fused.lm_head_logits(t_chunk(torch.cat([last[:, None], drafts], dim=1)), weight)  # [B (kk + 1), Vp]
        drawn = fused.lm_sample(t_logits, v, temperature, top_k, top_p, seed, next(steps))
        out = fused.speculative_verify(t_logits.view(B, kk + 1, -1), torch.stack(d_logits, dim=1), drafts.to(torch.int32),
                                       drawn.floor.view(B, kk + 1), torch.stack(d_floor, dim=1),
                                       drawn.ids.view(B, kk + 1)[:, kk], v, temperature, seed, next(steps))
        a = out.accepted.long()
        emitted = torch.cat([drafts, drafts[:, :1]], dim=1).scatter(1, a[:, None], out.next.long()[:, None])
        return drafts, emitted, a

    def _beam_search(self, input_ids, ids, lens, lo, n, eos, pad_token_id, nb, n_ret, length_penalty, early_stopping,
                     kv_cache_dtype=None, prefill_chunk_size=None, shared=False):
        """transformers' ``GenerationMixin._beam_search`` on the native cache: the same running / finished beam
        sets, scores and stopping rules, with two differences in mechanics.  The candidates of a step are the
        ``keep`` best continuations of every beam (``fused.lm_head_topk``: values - logsumexp are the
        log-probabilities) instead of a [B, num_beams * V] log-softmax -- a beam's continuation outside its own
        best ``keep`` cannot be among the batch row's best ``keep``.  And the prompt is prefilled once per row,
        its cache rows repeated (``KVCache.repeat_rows``), and every step moves only the generated suffix
        between the beams of a row (``KVCache.reorder_rows``).  One host read per step (HF reads the same flag).
        ``shared``: the prefill's cache is not repeated; the beams share it through a :class:`BeamKVCache`."""
        B, T0 = input_ids.shape
        dev = input_ids.device
        cfg, weight, base = self.config, self.lm_head.weight, self._decoder()
        keep = max(2, 1 + (0 if eos is None else int(eos.numel()))) * nb
        if keep > fused.LM_TOPK_MAX or keep > cfg.vocab_size:
            raise ValueError(f"generate: num_beams = {nb} keeps {keep} candidates per beam; at most "
                             f"{min(fused.LM_TOPK_MAX, cfg.vocab_size)} (the top-k kernel's k, the vocabulary) fit")
        fill = pad_token_id if pad_token_id is not None else 0
        rows = torch.arange(B, device=dev)
        first = KVCache(cfg, B, T0 if shared else T0 + n, dev, weight.dtype, kv_cache_dtype)
        h = self._prefill(base, ids, lens, first, prefill_chunk_size)  # one prefill per prompt
        cache = BeamKVCache(first, nb, n, cfg, weight.dtype) if shared else first.repeat_rows(nb)
        del first
        h = h.repeat_interleave(nb, dim=0)

        run_seq = torch.full((B, nb, n), fill, dtype=torch.long, device=dev)
        fin_seq = run_seq.clone()
        run_scores = torch.zeros(B, nb, dtype=torch.float32, device=dev)
        run_scores[:, 1:] = -1e9  # the beams of a row start equal: only the first may be continued
        fin_scores = torch.full((B, nb), -1e9, dtype=torch.float32, device=dev)
        fin_done = torch.zeros(B, nb, dtype=torch.bool, device=dev)
        fin_len = torch.zeros(B, nb, dtype=torch.long, device=dev)
        unsat = torch.ones(B, 1, dtype=torch.bool, device=dev)  # the open beams may still beat the finished ones
        top_mask = torch.arange(keep, device=dev) < nb
        offset = (rows * nb)[:, None]
        for i in range(n):
            top = fused.lm_head_topk(h, weight, keep)
            logp = (top.values - top.lse[:, None]) + run_scores.view(-1, 1)
            cand_lp, pick = torch.topk(logp.view(B, nb * keep), keep)
            cand_beam = pick // keep
            tok = top.ids.view(B, nb * keep).gather(1, pick).long()
            cand_seq = run_seq.gather(1, cand_beam[:, :, None].expand(-1, -1, n))
            cand_seq[:, :, i] = tok
            if i + 1 == n:
                hits = torch.ones_like(tok, dtype=torch.bool)
            elif eos is not None:
                hits = torch.isin(tok, eos)
            else:
                hits = torch.zeros_like(tok, dtype=torch.bool)
            # the open beams of the next step: the best candidates that did not stop
            run_lp = cand_lp + hits.to(torch.float32) * -1.0e9
            nxt = torch.topk(run_lp, nb)[1]
            run_seq = cand_seq.gather(1, nxt[:, :, None].expand(-1, -1, n))
            run_scores = run_lp.gather(1, nxt)
            beam_idx = (cand_beam.gather(1, nxt) + offset).reshape(-1)
            # the finished set: candidates among the best num_beams that stopped, merged with the earlier ones
            did = hits & top_mask[None, :]
            fin_lp = cand_lp / ((i + 1) ** length_penalty)
            full = fin_done.all(dim=-1, keepdim=True) & (early_stopping is True)
            fin_lp = fin_lp + full.to(torch.float32) * -1.0e9
            fin_lp = fin_lp + (~unsat).to(torch.float32) * -1.0e9
            fin_lp = fin_lp + (~did) * -1.0e9
            m_scores = torch.cat((fin_scores, fin_lp), dim=1)
            best = torch.topk(m_scores, nb)[1]
            fin_seq = torch.cat((fin_seq, cand_seq), dim=1).gather(1, best[:, :, None].expand(-1, -1, n))
            fin_scores = m_scores.gather(1, best)
            fin_done = torch.cat((fin_done, did), dim=1).gather(1, best)
            fin_len = torch.cat((fin_len, torch.full_like(tok, i + 1)), dim=1).gather(1, best)
            # can an open beam still beat the worst finished one (HF's heuristic for early_stopping=False)?
            best_open = run_scores[:, :1] / ((i + 1) ** length_penalty)
            worst = torch.where(fin_done, fin_scores.min(dim=1, keepdim=True)[0], -1.0e9)
            unsat = unsat & torch.any(best_open > worst, dim=-1, keepdim=True)
            go_on = torch.any(unsat) & ~(torch.all(fin_done) & (early_stopping is True)) & ~torch.all(hits)
            if not bool(go_on):  # the one host read of the step
                break
            if shared:
                cache.reorder_rows(beam_idx)
            else:
                cache.reorder_rows(beam_idx, lo)
            h = base(run_seq[:, :, i].reshape(-1, 1), cache=cache)[:, 0]
        seqs = fin_seq[:, :n_ret].reshape(B * n_ret, n)
        n_new = int(fin_len[:, :n_ret].max())
        out = torch.cat([input_ids.repeat_interleave(n_ret, dim=0), seqs[:, :n_new]], dim=1)
        return GenerateOutput(out, fin_scores[:, :n_ret].reshape(-1))
