"""``generate(num_beams=3, beam_cache="shared")`` on the GPU in bf16 with the kernel-eligible tiny models of
tests/test_generate_gpu.py (GPT-2 at head_dim 64, Llama with GQA 4:1 at 128, a Mistral window of 32 that cuts inside
the longer prompt): every step runs csrc/prefix_attention.hip (the PyTorch forms are patched to fail), and the returned
scores match the fp32 twin's teacher-forced log-probabilities of the returned sequences within MAX_RATIO, the factor
tests/test_beam_search_gpu.py applies to the default path (docs/TEST_TOLERANCES.md "Beam search")."""
import pytest
import torch

from beam_cases import score_ratio
from distributed_lion_pytorch_amd.ops import fused, hip
from test_beam_search_cpu import tg_prompts
from test_generate_gpu import MAX_RATIO, pair

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", ["gpt2", "llama", "mistral"])
def test_shared_beam_search(family, cuda, monkeypatch):
    hip.require()
    for f in ("shared_prefix_attention_reference", "kv_append_suffix_reference", "_lm_topk_torch"):
        monkeypatch.setattr(fused, f, lambda *a, **kw: pytest.fail("a PyTorch form ran"))
    m, ref = pair(family, cuda)
    ids, mask = tg_prompts(cuda)
    T, n, nb = ids.shape[1], 12, 3
    kw = dict(attention_mask=mask, max_new_tokens=n, num_beams=nb, num_return_sequences=nb, beam_cache="shared",
              return_dict_in_generate=True)
    out = m.generate(ids, **kw)
    seq, scores = out.sequences, out.sequences_scores
    assert seq.shape == (2 * nb, T + n) and torch.equal(seq[:, :T], ids.repeat_interleave(nb, dim=0))
    again = m.generate(ids, **kw)
    assert torch.equal(again.sequences, seq) and torch.equal(again.sequences_scores, scores), "two calls, same bits"
    ratio = score_ratio(m, ref, ids, mask, seq, scores, nb, None, 1.0)
    print(f"[beam shared] {family}: |S - sum l32| / sum |l16 - l32| = {ratio:.3f}")
    assert ratio <= MAX_RATIO
    pieces = m.generate(ids, prefill_chunk_size=16, **kw)
    ratio = score_ratio(m, ref, ids, mask, pieces.sequences, pieces.sequences_scores, nb, None, 1.0)
    print(f"[beam shared] {family}, prefill in pieces of 16: ratio {ratio:.3f}")
    assert ratio <= MAX_RATIO
    fused.check_index_errors(blocking=True)
