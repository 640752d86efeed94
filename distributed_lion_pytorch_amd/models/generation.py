"""Generation for the native causal LMs: a token-major KV cache and ``generate``.

``KVCache`` holds, per layer, k / v buffers ``[B, max_len, Hkv, D]`` -- the layout the training path computes
k and v in, so the prefill writes them with plain copies -- and the per-row lengths on the device.  The models
take it as an optional ``cache`` argument (models/llama.py, models/gpt2.py): the first call is the prefill (the
prompt through the flash forward), every later call one decode step (one token per row through
``fused.kv_append`` and ``fused.decode_attention``, csrc/decode.hip) or a chunk of up to 8 tokens per row, ragged
by ``n_new`` (``fused.kv_append_chunk`` and ``fused.chunk_attention``, csrc/chunk_attention.hip);
``KVCache.truncate`` rolls rows back.

``NativeGenerateMixin.generate`` uses HF's argument names: greedy or sampled (temperature, then top-k, then
top-p), ragged prompts by ``attention_mask`` (left- or right-padded), EOS / pad handling; ``num_beams > 1`` is beam
search (HF's semantics) on ``fused.lm_head_topk``; ``assistant_model`` is greedy speculative decoding (a draft
model proposes, one chunk forward of this model checks).  Out of scope: beam sampling, diverse / constrained
beams, repetition penalties, a paged or rolling cache (a windowed layer keeps its full-length cache and only
bounds the key range), graph capture, speculative sampling.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from ..ops import fused
from ..ops.linear import gemm_fwd

_EOS_CHECK_EVERY = 8  # decode steps between two host reads of "every row has finished"


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

    def __init__(self, config, batch: int, max_len: int, device=None, dtype=torch.float32):
        layers, hkv, hd = cache_geometry(config)
        self.batch, self.max_len = int(batch), int(max_len)
        if self.batch < 1 or self.max_len < 1:
            raise ValueError("KVCache: batch and max_len must be positive")
        # one allocation: [layer, k | v, B, max_len, Hkv, D]
        self._buf = torch.zeros(layers, 2, self.batch, self.max_len, hkv, hd, device=device, dtype=dtype)
        self.lengths = torch.zeros(self.batch, dtype=torch.int32, device=device)
        self.kv_len = self.lengths  # lengths + 1 during a decode step
        self.width = 0
        self.prefilled = False
        self.chunk = False  # the forward in flight takes the chunk path (T > 1 tokens per row, or ragged)
        self.n_new = None  # int32 [B]: the tokens of the chunk in flight that row b keeps (None: all T)

    def layer(self, i: int):
        """(k, v) of layer i, each [B, max_len, Hkv, D]."""
        return self._buf[i, 0], self._buf[i, 1]

    def begin(self, B: int, T: int, n_new: Optional[torch.Tensor] = None) -> bool:
        """Start a forward of T tokens per row; True for the prefill (the first call).  After the prefill T = 1
        is a decode step and 1 < T <= 8 a chunk (``fused.kv_append_chunk`` / ``fused.chunk_attention``), of
        which row b keeps the first ``n_new[b]`` tokens ([B], 0 <= n_new[b] <= T; None: all T)."""
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
        if not 1 <= T <= fused.CHUNK_MAX_TOKENS:
            raise ValueError(f"KVCache: after the prefill a forward takes 1 to {fused.CHUNK_MAX_TOKENS} tokens per row")
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
        out.batch, out.max_len = self.batch * n, self.max_len
        shape = list(self._buf.shape)
        shape[2] = out.batch
        out._buf = torch.zeros(shape, device=self._buf.device, dtype=self._buf.dtype)
        w = self.width
        out._buf[:, :, :, :w] = self._buf[:, :, :, :w].repeat_interleave(n, dim=2)
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
            part = self._buf[:, :, :, lo:self.width]
            self._buf[:, :, :, lo:self.width] = part.index_select(2, index)
        self.lengths.copy_(self.lengths.index_select(0, index))


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
                 assistant_model=None, num_assistant_tokens: int = 5):
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
        :class:`SpeculativeOutput`."""
        num_beams, num_return_sequences = int(num_beams), int(num_return_sequences)
        if num_beams < 1:
            raise ValueError("generate: num_beams must be >= 1")
        if num_return_sequences < 1 or num_return_sequences > num_beams:
            raise ValueError("generate: num_return_sequences must be in [1, num_beams]"
                             + (" (more than one sequence per prompt needs num_beams > 1)" if num_beams == 1 else ""))
        if num_beams > 1 and do_sample:
            raise ValueError("generate: num_beams > 1 with do_sample=True (beam sampling) is not supported")
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
            if do_sample or num_beams != 1:
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
            out = self._speculative(assistant_model, input_ids, ids, lens, max_new_tokens, eos, pad_token_id, k)
            fused.check_index_errors()
            return out if return_dict_in_generate else out.sequences
        if num_beams > 1:
            lo = T0 if attention_mask is None else int(lens.min())
            out = self._beam_search(input_ids, ids, lens, lo, max_new_tokens, eos, pad_token_id, num_beams,
                                    num_return_sequences, float(length_penalty), early_stopping)
            fused.check_index_errors()
            return out if return_dict_in_generate else out.sequences
        cache = KVCache(cfg, B, total, dev, weight.dtype)
        gen = None
        if do_sample and seed is not None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed))

        base = self._decoder()
        rows = torch.arange(B, device=dev)
        h = base(ids, cache=cache)[rows, lens - 1]  # prefill: the hidden state of every row's last real token
        cache.set_lengths(lens)
        new = torch.empty(B, max_new_tokens, dtype=torch.long, device=dev)
        finished = torch.zeros(B, dtype=torch.bool, device=dev)
        done_at = torch.full((B,), max_new_tokens, dtype=torch.long, device=dev)  # the step a row emitted EOS at
        ignore = torch.full((B,), -100, dtype=torch.long, device=dev)
        for i in range(max_new_tokens):
            if do_sample:
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

    def _speculative(self, assistant, input_ids, ids, lens, n, eos, pad_token_id, k):
        """Greedy speculative decoding.  Row b has emitted ``count[b]`` tokens, the last of which (``last``) is not
        in the target's cache yet; the assistant's cache lacks the last one or two of them (``unseen``: two when
        every draft of the previous round was accepted, since the last draft was never fed to the assistant).  A
        round: the assistant absorbs ``unseen`` in a ragged chunk of 2 and drafts kk tokens (kk - 1 single-token
        steps), the target runs one chunk of ``last`` and the drafts, row b keeps the ``a[b]`` drafts that equal the
        target's top-1 and the target's next token, and both caches are rolled back to what stays valid.  Rows
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
        cache = KVCache(cfg, B, size, dev, weight.dtype)
        a_cache = KVCache(acfg, B, size, dev, a_weight.dtype)
        h = base(ids, cache=cache)[rows, lens - 1]
        cache.set_lengths(lens)
        a_base(ids, cache=a_cache)
        a_cache.set_lengths(lens)

        def top1(hidden, w):
            flat = hidden.reshape(-1, hidden.shape[-1])
            return fused.lm_head_score(flat, w, torch.full((flat.shape[0],), -100, dtype=torch.long, device=dev)).pred.long()

        new = torch.zeros(B, n + k + 1, dtype=torch.long, device=dev)
        last = top1(h, weight)
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
            drafts = [top1(ha[rows, (n_unseen - 1).clamp_min(0)], a_weight)]
            for _ in range(kk - 1):
                drafts.append(top1(a_base(drafts[-1][:, None], cache=a_cache)[:, 0], a_weight))
            drafts = torch.stack(drafts, dim=1)  # [B, kk]
            # the target: one chunk over the last emitted token and the drafts
            chunk = torch.cat([last[:, None], drafts], dim=1)
            pred = top1(base(chunk, cache=cache), weight).view(B, kk + 1)  # the target's token after each of the chunk's inputs
            a = (pred[:, :kk] == drafts).long().cumprod(1).sum(1)  # accepted drafts
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

    def _beam_search(self, input_ids, ids, lens, lo, n, eos, pad_token_id, nb, n_ret, length_penalty, early_stopping):
        """transformers' ``GenerationMixin._beam_search`` on the native cache: the same running / finished beam
        sets, scores and stopping rules, with two differences in mechanics.  The candidates of a step are the
        ``keep`` best continuations of every beam (``fused.lm_head_topk``: values - logsumexp are the
        log-probabilities) instead of a [B, num_beams * V] log-softmax -- a beam's continuation outside its own
        best ``keep`` cannot be among the batch row's best ``keep``.  And the prompt is prefilled once per row,
        its cache rows repeated (``KVCache.repeat_rows``), and every step moves only the generated suffix
        between the beams of a row (``KVCache.reorder_rows``).  One host read per step (HF reads the same flag)."""
        B, T0 = input_ids.shape
        dev = input_ids.device
        cfg, weight, base = self.config, self.lm_head.weight, self._decoder()
        keep = max(2, 1 + (0 if eos is None else int(eos.numel()))) * nb
        if keep > fused.LM_TOPK_MAX or keep > cfg.vocab_size:
            raise ValueError(f"generate: num_beams = {nb} keeps {keep} candidates per beam; at most "
                             f"{min(fused.LM_TOPK_MAX, cfg.vocab_size)} (the top-k kernel's k, the vocabulary) fit")
        fill = pad_token_id if pad_token_id is not None else 0
        rows = torch.arange(B, device=dev)
        first = KVCache(cfg, B, T0 + n, dev, weight.dtype)
        h = base(ids, cache=first)[rows, lens - 1]  # one prefill per prompt
        first.set_lengths(lens)
        cache = first.repeat_rows(nb)
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
            cache.reorder_rows(beam_idx, lo)
            h = base(run_seq[:, :, i].reshape(-1, 1), cache=cache)[:, 0]
        seqs = fin_seq[:, :n_ret].reshape(B * n_ret, n)
        n_new = int(fin_len[:, :n_ret].max())
        out = torch.cat([input_ids.repeat_interleave(n_ret, dim=0), seqs[:, :n_new]], dim=1)
        return GenerateOutput(out, fin_scores[:, :n_ret].reshape(-1))
