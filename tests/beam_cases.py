"""Shared by the beam-search tests: a naive beam search that re-runs the full forward on the growing sequences
(no cache, a full log-softmax over [B, num_beams * V]) and the score check of a returned beam against the
teacher-forced log-probabilities of the fp32 twin."""
import torch

from distributed_lion_pytorch_amd.ops import fused


@torch.no_grad()
def naive_beam_search(model, ids, n, nb, n_ret=1, length_penalty=1.0, early_stopping=False, eos=None, pad=0):
    """(sequences [B * n_ret, T0 + n_new], scores [B * n_ret]) for equal-length prompts: transformers' beam search
    (running and finished sets of num_beams, max(2, 1 + #eos) * num_beams candidates per step) written on the
    whole vocabulary, with the model re-run on every beam's whole sequence at every step."""
    B, T0 = ids.shape
    V = model.config.vocab_size
    eos_t = None if eos is None else torch.as_tensor([eos] if isinstance(eos, int) else list(eos))
    keep = max(2, 1 + (0 if eos_t is None else len(eos_t))) * nb
    run = torch.full((B, nb, T0 + n), pad, dtype=torch.long)
    run[:, :, :T0] = ids[:, None]
    fin = run.clone()
    run_sc = torch.zeros(B, nb)
    run_sc[:, 1:] = -1e9
    fin_sc = torch.full((B, nb), -1e9)
    fin_done = torch.zeros(B, nb, dtype=torch.bool)
    fin_len = torch.zeros(B, nb, dtype=torch.long)
    unsat = torch.ones(B, 1, dtype=torch.bool)
    for i in range(n):
        cur = T0 + i
        logits = model(run[:, :, :cur].reshape(B * nb, cur)).logits[:, -1].float()
        logp = torch.log_softmax(logits, -1).view(B, nb, V) + run_sc[:, :, None]
        lp, pick = torch.topk(logp.view(B, nb * V), keep)
        cand = run.gather(1, (pick // V)[:, :, None].expand(-1, -1, T0 + n))
        cand[:, :, cur] = pick % V
        hits = torch.isin(pick % V, eos_t) if eos_t is not None else torch.zeros_like(pick, dtype=torch.bool)
        if i + 1 == n:
            hits = torch.ones_like(hits)
        run_lp = lp + hits.float() * -1e9
        nxt = torch.topk(run_lp, nb)[1]
        run = cand.gather(1, nxt[:, :, None].expand(-1, -1, T0 + n))
        run_sc = run_lp.gather(1, nxt)
        did = hits & (torch.arange(keep) < nb)[None]
        f = lp / ((i + 1) ** length_penalty)
        f = f + (fin_done.all(-1, keepdim=True) & (early_stopping is True)).float() * -1e9
        f = f + (~unsat).float() * -1e9
        f = f + (~did) * -1e9
        ms = torch.cat((fin_sc, f), 1)
        best = torch.topk(ms, nb)[1]
        fin = torch.cat((fin, cand), 1).gather(1, best[:, :, None].expand(-1, -1, T0 + n))
        fin_sc = ms.gather(1, best)
        fin_done = torch.cat((fin_done, did), 1).gather(1, best)
        fin_len = torch.cat((fin_len, torch.full_like(pick, i + 1)), 1).gather(1, best)
        worst = torch.where(fin_done, fin_sc.min(1, keepdim=True)[0], -1e9)
        unsat = unsat & torch.any(run_sc[:, :1] / ((i + 1) ** length_penalty) > worst, -1, keepdim=True)
        if not bool(unsat.any()) or (early_stopping and bool(fin_done.all())) or bool(hits.all()):
            break
    n_new = int(fin_len[:, :n_ret].max())
    return fin[:, :n_ret, :T0 + n_new].reshape(B * n_ret, -1), fin_sc[:, :n_ret].reshape(-1)


def generated_lengths(new, eos):
    """Tokens generated per row up to and including its first EOS (all of them without one)."""
    n = torch.full((new.shape[0],), new.shape[1], dtype=torch.long)
    if eos is not None:
        for r in range(new.shape[0]):
            hit = (new[r] == eos).nonzero()
            if len(hit):
                n[r] = int(hit[0]) + 1
    return n


@torch.no_grad()
def teacher_forced_logprobs(model, seq, start, torch_forms=False):
    """log-probabilities [rows, L - start] of seq[:, start:] given everything before, from the full forward on
    seq [rows, L] (no cache), log-softmax in fp32."""
    if torch_forms:
        fused.set_impl("torch")
    try:
        logits = model(seq).logits.float()
    finally:
        if torch_forms:
            fused.set_impl("auto")
    lp = torch.log_softmax(logits[:, start - 1:-1], -1)
    return lp.gather(-1, seq[:, start:, None])[..., 0]


def score_ratio(m16, m32, ids, mask, out, scores, n_ret, eos, length_penalty):
    """max over the returned sequences of |S - sum(l32)| / sum(|l16 - l32|), S = score * n ** length_penalty, n the
    tokens generated up to and including the EOS; l32 / l16 the teacher-forced log-probabilities of those tokens
    from the fp32 twin (PyTorch forms) and from the full forward of the model that generated.  ``out`` is
    [B * n_ret, T0 + n_new] for the prompts ids [B, T0] with their mask."""
    T0 = ids.shape[1]
    worst = 0.0
    for b in range(ids.shape[0]):
        rows = slice(b * n_ret, (b + 1) * n_ret)
        real = ids[b][mask[b] != 0]
        k = real.numel()
        seq = torch.cat([real[None].expand(n_ret, -1), out[rows, T0:]], dim=1)  # the padding dropped
        n = generated_lengths(seq[:, k:], eos).to(out.device)
        l32 = teacher_forced_logprobs(m32, seq, k, torch_forms=True).double()
        l16 = teacher_forced_logprobs(m16, seq, k).double()
        live = torch.arange(seq.shape[1] - k, device=out.device)[None] < n[:, None]
        S = scores[rows].double() * n.double() ** length_penalty
        lhs = (S - (l32 * live).sum(1)).abs()
        rhs = ((l16 - l32).abs() * live).sum(1)
        worst = max(worst, float((lhs / rhs).max()))
    return worst
