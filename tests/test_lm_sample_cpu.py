"""The PyTorch form of the LM-head sampling kernel (fused._lm_sample_torch) against the fp64 contract of
tests/lm_sample_cases.py; the reference itself leaves the GPU test's cases no freedom (floor forced, token
decided); generate(sampler="fused") on tiny native models; generate.py --sampler."""
import pytest
import torch

import lm_sample_cases as sc
import test_generate_cpu as tg
from distributed_lion_pytorch_amd.models.generation import warp_logits
from distributed_lion_pytorch_amd.ops import fused

SMALL = [(dt, v) for dt in sc.DTYPES for v in sc.VOCABS if v <= 4099]


def distribution_is_softmax(sample):
    """N = 16384 equal rows of 8 logits, nothing filtered: the token counts against the fp64 softmax, within 5
    binomial standard deviations per column.  ``sample(x) -> ids``; the rows differ by their index in the hash."""
    n = 16384
    x = torch.tensor([0.5, -1.0, 2.0, 0.0, 1.5, -3.0, 1.0, -0.25]).repeat(n, 1)
    p = x[0].double().softmax(-1)
    counts = torch.bincount(sample(x).long().cpu(), minlength=8).double()
    assert int(counts.sum()) == n and counts.numel() == 8
    assert bool(((counts - n * p).abs() <= 5 * (n * p * (1 - p)).sqrt()).all()), (counts / n, p)


@pytest.mark.parametrize("dtype,v", SMALL, ids=[f"{str(d)[6:]}-{v}" for d, v in SMALL])
def test_torch_form_against_fp64(dtype, v):
    for n in (1, 3):
        for setting in sc.SETTINGS:
            x, inv_t, k, p, ref = sc.case(n, v, dtype, setting)
            sc.check(fused._lm_sample_torch(x, v, inv_t, k, p, sc.KEY), x, v, inv_t, k, p, ref, f"{dtype} {v} {n} {setting}")


def test_reference_leaves_no_freedom():
    """Over every case of the GPU test: one floor value meets the mass bound and the runner-up token is more than
    2 delta away on at least 90 % of the (case, row) pairs, judged on the reference's own best token."""
    stats = []
    for dtype in sc.DTYPES:
        for v in sc.VOCABS:
            for n in (1, 3):
                for setting in sc.SETTINGS:
                    x, inv_t, k, p, ref = sc.case(n, v, dtype, setting)
                    stats += sc.check(fused._lm_sample_torch(x, v, inv_t, k, p, sc.KEY), x, v, inv_t, k, p, ref, "ref")
    sharp, decided = (sum(s[i] for s in stats) / len(stats) for i in (0, 1))
    print(f"floor forced on {sharp:.3f}, token decided on {decided:.3f} of {len(stats)} rows")
    assert sharp >= 0.9 and decided >= 0.9


@pytest.mark.parametrize("setting", [(0.7, 50, 1.0), (1.3, 0, 0.9), (0.8, 40, 0.95)])
def test_survivors_are_warp_logits_survivors(setting):
    t, k, p = setting
    x = sc.rows(3, 513, torch.float32, seed=2)
    s = x[:, :513] * sc.inv_temperature(t)
    assert all(r.unique().numel() == 513 for r in s), "tie-free rows"
    _, _, floor, kept = fused._lm_sample_torch(x, 513, sc.inv_temperature(t), k, p, sc.KEY)
    want = warp_logits(x[:, :513], t, k, p) != float("-inf")
    assert torch.equal(s >= floor[:, None], want) and torch.equal(kept.long(), want.sum(1))


def test_distribution():
    distribution_is_softmax(lambda x: fused._lm_sample_torch(x, 8, 1.0, 0, 1.0, sc.KEY)[0])


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_generate_with_the_fused_sampler(family):
    m = tg.model_of(family)
    ids = tg._prompts(m, 3, 5)
    kw = dict(max_new_tokens=8, do_sample=True, temperature=0.9, top_k=7, top_p=0.95)
    a = m.generate(ids, sampler="fused", seed=3, **kw)
    assert torch.equal(a, m.generate(ids, sampler="fused", seed=3, **kw))
    assert not torch.equal(a, m.generate(ids, sampler="fused", seed=4, **kw))
    with torch.no_grad():
        logits = m(a[:, :-1]).logits[:, 4:].float()  # teacher-forced: the logits every new token was drawn from
    top = logits.topk(7, dim=-1).indices
    assert bool((top == a[:, 5:, None]).any(-1).all()), "a token outside the top-k set"
    assert torch.equal(m.generate(ids, seed=3, **kw), m.generate(ids, sampler="torch", seed=3, **kw))


def test_sampler_refusals():
    m = tg.model_of("llama")
    ids = tg._prompts(m, 2, 4)
    for kw in (dict(do_sample=False), dict(do_sample=True, num_beams=2), dict(assistant_model=tg.model_of("llama"))):
        with pytest.raises(ValueError, match="sampler='fused'"):
            m.generate(ids, max_new_tokens=2, sampler="fused", **kw)
    with pytest.raises(ValueError, match="sampler"):
        m.generate(ids, max_new_tokens=2, do_sample=True, sampler="gumbel")


def test_generate_py_sampler_flag():
    import generate

    cli = ["--model_name_or_path", "gpt2-tiny", "--config_overrides", "n_layer=1,n_embd=32,n_head=2", "--prompt", "ab",
           "--max_new_tokens", "5", "--device", "cpu", "--do_sample", "--top_k", "9", "--seed", "1", "--sampler", "fused"]
    out = generate.main(cli)
    assert out.shape == (1, 2 + 5) and out[0, :2].tolist() == [97, 98]
