"""Speculative sampling on the CPU: fused._spec_verify_torch against the fp64 contract of tests/spec_verify_cases.py on
every case of the GPU test (which also asserts the cases are decided), the emitted token's distribution,
generate(sampler="speculative") with top_k=1 against plain greedy decoding, the refusals, generate.py's flag."""
import pytest
import torch

import spec_verify_cases as sv
import test_speculative_cpu as ts
from distributed_lion_pytorch_amd.models.generation import SpeculativeOutput
from distributed_lion_pytorch_amd.ops import fused

CASES = [(dt, v) for dt in sv.DTYPES for v in sv.VOCABS]


@pytest.mark.parametrize("dtype,v", CASES, ids=[f"{str(d)[6:]}-{v}" for d, v in CASES])
def test_torch_form_against_fp64(dtype, v):
    for c in sv.all_cases(dtype, v):
        args, ref = sv.case(*c)
        sv.check(fused._spec_verify_torch(*args), args, ref, str(c), same=c[4])


def test_distribution():
    sv.distribution_is_the_targets(fused._spec_verify_torch)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_top_k_1_is_plain_greedy(family):
    """Ragged prompts and an EOS; every distribution is a point mass, so the tokens are the greedy ones."""
    m = ts.model_of(family)
    T0, n = 10, 14
    ids = ts._prompts(3, T0, seed=2)
    mask = torch.ones_like(ids)
    mask[0, :4] = 0
    free = m.generate(ids, attention_mask=mask, max_new_tokens=n)
    kw = dict(attention_mask=mask, max_new_tokens=n, eos_token_id=int(free[1, T0 + 2]), pad_token_id=96)
    plain = m.generate(ids, **kw)
    for name, a in ts.assistants(family).items():
        for k in (1, 5):
            out = m.generate(ids, assistant_model=a, num_assistant_tokens=k, do_sample=True, top_k=1, sampler="speculative",
                             seed=5, return_dict_in_generate=True, **kw)
            assert isinstance(out, SpeculativeOutput) and torch.equal(out.sequences, plain), (family, name, k)


def test_refusals():
    m, a = ts.model_of("llama"), ts.model_of("llama", 1, 1)
    ids = ts._prompts(2, 4)
    for kw in (dict(do_sample=False, assistant_model=a), dict(do_sample=True), dict(do_sample=True, assistant_model=a, num_beams=2)):
        with pytest.raises(ValueError, match="sampler='speculative'"):
            m.generate(ids, max_new_tokens=2, sampler="speculative", **kw)
    with pytest.raises(ValueError, match="do_sample=False"):
        m.generate(ids, max_new_tokens=2, assistant_model=a, do_sample=True)
    with pytest.raises(ValueError, match="sampler='fused'"):
        m.generate(ids, max_new_tokens=2, assistant_model=a, do_sample=True, sampler="fused")
    args, _ = sv.case(13, torch.float32, sv.SETTINGS[3], (3, 4), False)
    with pytest.raises(ValueError, match="speculative_verify needs"):
        fused.speculative_verify(args[0][:, :4], *args[1:7])
    with pytest.raises(ValueError, match="num_assistant_tokens"):
        m.generate(ids, max_new_tokens=2, assistant_model=a, do_sample=True, sampler="speculative", num_assistant_tokens=8)


def test_generate_py_sampler_flag(capsys):
    import generate

    cli = ["--model_name_or_path", "gpt2-tiny", "--config_overrides", "n_layer=1,n_embd=32,n_head=2", "--prompt", "ab",
           "--max_new_tokens", "5", "--device", "cpu", "--do_sample", "--top_k", "9", "--seed", "1", "--sampler", "speculative",
           "--assistant_model", "gpt2-tiny", "--num_assistant_tokens", "3"]
    out = generate.main(cli)
    assert out.shape == (1, 2 + 5) and out[0, :2].tolist() == [97, 98]
    assert "[generate] speculative: " in capsys.readouterr().out
