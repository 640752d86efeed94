"""The verify kernel (csrc/spec_verify.hip) and ``fused.speculative_verify`` on the GPU against the fp64 form of the
contract (tests/spec_verify_cases.py), bit-equal repeats and a clean arrival workspace; the emitted token's
distribution; generate(sampler="speculative") on the tiny bf16 models of the speculative test."""
import pytest
import torch

import spec_verify_cases as sv
import test_speculative_gpu as sg
from distributed_lion_pytorch_amd.ops import fused, hip

pytestmark = pytest.mark.gpu

CASES = [(dt, v) for dt in sv.DTYPES for v in sv.VOCABS]


def run_kernel(args, dev, arrive):
    T, D, drafts, t_floor, d_floor, bonus, v, inv_t, key = args
    return hip.ops().spec_verify(T.to(dev), D.to(dev), drafts.to(dev), t_floor.to(dev), d_floor.to(dev), bonus.to(dev), v,
                                 inv_t, key, arrive)


@pytest.mark.parametrize("dtype,v", CASES, ids=[f"{str(d)[6:]}-{v}" for d, v in CASES])
def test_kernel_against_fp64(dtype, v, cuda):
    hip.require()
    arrive = torch.zeros(8, dtype=torch.int32, device=cuda)
    for c in sv.all_cases(dtype, v):
        args, ref = sv.case(*c)
        out = run_kernel(args, cuda, arrive)
        sv.check(out, args, ref, str(c), same=c[4])
        for a, b in zip(out, run_kernel(args, cuda, arrive)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "same inputs, same bits"
        assert not bool(arrive.any()), "the arrival counters are zero after a launch"


def test_distribution(cuda):
    hip.require()
    arrive = torch.zeros(8192, dtype=torch.int32, device=cuda)
    sv.distribution_is_the_targets(lambda *args: run_kernel(args, cuda, arrive))


def test_public_op_and_refusals(cuda, monkeypatch):
    hip.require()
    args, ref = sv.case(4099, torch.bfloat16, sv.SETTINGS[3], (3, 4), False)
    monkeypatch.setattr(fused, "_spec_verify_torch", lambda *a, **kw: pytest.fail("PyTorch spec_verify ran"))
    monkeypatch.setattr(fused, "_lm_sample_torch", lambda *a, **kw: pytest.fail("PyTorch lm_sample ran"))
    T, D, drafts, t_floor, d_floor, bonus, v, inv_t, key = (a.to(cuda) if torch.is_tensor(a) else a for a in args)
    out = fused.speculative_verify(T, D, drafts, t_floor, d_floor, bonus, v, temperature=0.8, seed=11, step=2)
    sv.check(out, args, ref, "public op")
    drawn = fused.lm_sample(D.view(-1, D.shape[-1]), v, 0.8, 50, 0.95, seed=11, step=0)  # on a block the caller keeps
    want = hip.ops().lm_sample(D.view(-1, D.shape[-1]), v, inv_t, 50, 0.95, sv.KEY_D)
    assert all(torch.equal(a, b) for a, b in zip(drawn, want)) and drawn.ids.shape == (12,)
    outside = drafts.clone()
    outside[0, 0], outside[1, 0] = -1, v  # a pad column's logit is 3e4: read, it would be accepted
    far = fused.speculative_verify(T, D, outside, t_floor, d_floor, bonus, v, temperature=0.8, seed=11, step=2)
    assert far.flags[:2, 0].tolist() == [0, 0] and far.accepted[:2].tolist() == [0, 0]
    arrive = torch.zeros(8, dtype=torch.int32, device=cuda)
    for bad in (dict(T=T.float()), dict(T=T[:, :4]), dict(D=torch.cat([D, D], 1)), dict(v=D.shape[-1] + 1), dict(key=2 ** 32),
                dict(drafts=drafts.long()), dict(arrive=arrive[:2]), dict(T=T[..., :4100], D=D[..., :4100])):
        a = {**dict(T=T, D=D, drafts=drafts, v=v, key=key, arrive=arrive), **bad}
        with pytest.raises(RuntimeError, match="dlion"):
            hip.ops().spec_verify(a["T"], a["D"], a["drafts"], t_floor, d_floor, bonus, a["v"], inv_t, a["key"], a["arrive"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_generate_with_speculative_sampling(family, cuda, monkeypatch):
    hip.require()
    sg.kernels_only(monkeypatch)
    monkeypatch.setattr(fused, "_spec_verify_torch", lambda *a, **kw: pytest.fail("PyTorch spec_verify ran"))
    m, _ = sg.target(family, cuda)
    small = sg.assistants(family, cuda)["one layer"]
    ids, mask, free, prefix = sg.plain_run(family, cuda)
    kw = dict(attention_mask=mask, max_new_tokens=sg.NEW, do_sample=True, sampler="speculative", return_dict_in_generate=True)
    warp = dict(temperature=0.9, top_k=20, top_p=0.95)
    out = m.generate(ids, assistant_model=small, seed=3, **warp, **kw)
    assert out.sequences.shape == free.shape and torch.equal(out.sequences[:, :sg.T0], ids)
    assert torch.equal(out.sequences, m.generate(ids, assistant_model=small, seed=3, **warp, **kw).sequences)
    own = m.generate(ids, assistant_model=m, seed=3, **warp, **kw)
    full, rest = divmod(sg.NEW - 1, 6)  # every draft offered is accepted: rounds of 5 drafts and one more token
    assert own.rounds == full + (rest > 0) and own.accepted.tolist() == [full * 5 + rest] * 3, (own.rounds, own.accepted)
    greedy = m.generate(ids, assistant_model=small, seed=3, top_k=1, **kw)
    sg.assert_same_where_decided(greedy.sequences, free, prefix, f"{family} / top_k = 1")
    cold = m.generate(ids, assistant_model=small, seed=3, kv_cache_dtype="fp8_e4m3", **warp, **kw)
    assert cold.sequences.shape == free.shape and int(cold.sequences.min()) >= 0
    fused.check_index_errors(blocking=True)
