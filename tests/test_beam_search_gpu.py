"""Beam search on the GPU in bf16 with the kernel-eligible tiny models of tests/test_generate_gpu.py: every step's
candidates come from csrc/lm_topk.hip and the decode kernels (the PyTorch forms are patched to fail), at 8 rows
(the skinny GEMM) and at 18 rows (the general dispatch).  Shape, prompt, repeatability, distinct beams, ordered
scores, EOS / pad; and the returned scores against the teacher-forced log-probabilities of the fp32 twin, within
the project's factor for "cached path versus full forward" (docs/TEST_TOLERANCES.md "Beam search")."""
import pytest
import torch

from beam_cases import generated_lengths, score_ratio
from distributed_lion_pytorch_amd.ops import fused, hip
from test_beam_search_cpu import tg_prompts
from test_generate_gpu import MAX_RATIO, _kernels_only, pair

pytestmark = pytest.mark.gpu

PAD = 255
CASES = [("gpt2", 2, 4), ("llama", 2, 4), ("mistral", 2, 4), ("llama", 6, 3)]  # 8 rows; 18 rows for the last


@pytest.mark.parametrize("family,B,nb", CASES, ids=[f"{f}-{B}x{nb}" for f, B, nb in CASES])
def test_beam_search(family, B, nb, cuda, monkeypatch):
    hip.require()
    _kernels_only(monkeypatch)
    monkeypatch.setattr(fused, "_lm_topk_torch", lambda *a, **kw: pytest.fail("PyTorch lm_topk ran"))
    m, ref = pair(family, cuda)
    ids, mask = tg_prompts(cuda, B=B)
    T, n = ids.shape[1], 12
    kw = dict(attention_mask=mask, max_new_tokens=n, num_beams=nb, num_return_sequences=nb, return_dict_in_generate=True)
    free = m.generate(ids, **kw)
    seq, scores = free.sequences, free.sequences_scores
    assert seq.shape == (B * nb, T + n) and seq.dtype == torch.long and scores.shape == (B * nb,)
    assert torch.equal(seq[:, :T], ids.repeat_interleave(nb, dim=0)), "the prompt comes back as given"
    assert int(seq.min()) >= 0 and int(seq.max()) < 256
    again = m.generate(ids, **kw)
    assert torch.equal(again.sequences, seq) and torch.equal(again.sequences_scores, scores), "two calls, same bits"
    for b in range(B):
        rows = seq[b * nb:(b + 1) * nb, T:]
        assert len({tuple(r.tolist()) for r in rows}) == nb, "the beams of a row are distinct"
        s = scores[b * nb:(b + 1) * nb]
        assert bool((s[1:] <= s[:-1]).all()), "best beam first"
    ratio = score_ratio(m, ref, ids, mask, seq, scores, nb, None, 1.0)
    print(f"[beam] {family} B={B} beams={nb}: |S - sum l32| / sum |l16 - l32| = {ratio:.3f}")
    assert ratio <= MAX_RATIO

    # an EOS from the free run: the best beam of row 0 stops at its third token; length_penalty != 1
    eos = int(seq[0, T + 2])
    out = m.generate(ids, eos_token_id=eos, pad_token_id=PAD, length_penalty=0.6, **kw)
    new = out.sequences[:, T:]
    lens = generated_lengths(new, eos)
    assert int(lens.min()) < n, "no beam finished early"
    for r in range(new.shape[0]):
        assert bool((new[r, int(lens[r]):] == PAD).all()), "every token after a row's EOS is the pad id"
    assert torch.equal(out.sequences[:, :T], ids.repeat_interleave(nb, dim=0))
    ratio = score_ratio(m, ref, ids, mask, out.sequences, out.sequences_scores, nb, eos, 0.6)
    print(f"[beam] {family} B={B} beams={nb}, EOS, length_penalty 0.6: ratio {ratio:.3f}")
    assert ratio <= MAX_RATIO
    fused.check_index_errors(blocking=True)
