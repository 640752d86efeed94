"""Opt-in stochastic rounding of the bf16 parameter store (CPU): the rounding
rule, the coordinate hash, the unfrozen weights, the dtype rules, replica
identity over gloo, the entrypoint flag and the kernels' register budget."""
import math
import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist

from dist_utils import run_world
from distributed_lion_pytorch_amd import Lion
from distributed_lion_pytorch_amd.ops import reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bits(x: torch.Tensor) -> torch.Tensor:
    return x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF


# ------------------------------------------------------------ 1. sr_bf16
def test_sr_bf16_keeps_representable_values():
    largest = torch.tensor([0x7F7F0000], dtype=torch.int32).view(torch.float32).item()  # largest normal below Inf
    x = torch.tensor([0.0, -0.0, 0.5, -0.25, largest, -largest], dtype=torch.float32)
    for r in (0, 65535):
        out = ref.sr_bf16(x, torch.full((x.numel(),), r, dtype=torch.int64))
        assert out.dtype == torch.bfloat16
        assert torch.equal(_bits(out.float()), _bits(x)), r  # bit patterns: -0 stays -0


@pytest.mark.parametrize("value", [1.0001, -1.0001, 0.1, -0.3333, 3.0e-5, -7.77e20, 0.99999])
def test_sr_bf16_two_neighbours_and_exact_up_count(value):
    x = torch.tensor([value], dtype=torch.float32)
    b = int(_bits(x))
    low = b & 0xFFFF
    assert low != 0, "pick a value that bf16 does not represent"
    r = torch.arange(65536, dtype=torch.int64)
    out = _bits(ref.sr_bf16(x.expand(65536).contiguous(), r).float())
    down, up = b & 0xFFFF0000, (b & 0xFFFF0000) + 0x10000  # toward zero / away from zero (sign-magnitude)
    assert set(out.unique().tolist()) == {down, up}
    assert int((out == up).sum()) == low
    # unbiased: the mean over all r is x up to the fp64 sum's rounding
    vals = out.to(torch.int32).view(torch.float32).double()
    assert abs(vals.mean().item() - x.double().item()) <= abs(value) * 2.0 ** -40


def test_sr_bf16_nan_inf_pass_through():
    x = torch.tensor([float("inf"), float("-inf"), float("nan")], dtype=torch.float32)
    out = ref.sr_bf16(x, torch.full((3,), 65535, dtype=torch.int64))
    assert out[0] == float("inf") and out[1] == float("-inf") and torch.isnan(out[2])


# --------------------------------------------------------------- 2. hash
def test_sr_bits_uniform_fresh_and_deterministic():
    n = 1 << 16
    for base in (0, 8 * 123_456_789 * 8, (1 << 33) + 2048):  # a 64-bit coordinate too
        c = base + torch.arange(n, dtype=torch.int64)
        r = ref.sr_bits16(c, seed=3, step=17)
        assert r.dtype == torch.int64 and int(r.min()) >= 0 and int(r.max()) < 65536
        assert abs((r.double() / 65536).mean().item() - 0.5) < 5 / math.sqrt(12 * n)
        assert torch.equal(r, ref.sr_bits16(c, seed=3, step=17))  # a pure function
        assert (r != ref.sr_bits16(c, seed=3, step=18)).double().mean().item() > 0.99
        assert (r != ref.sr_bits16(c, seed=4, step=17)).double().mean().item() > 0.99
    # the two halves of a pair's hash: even and odd coordinates are different streams
    c = torch.arange(n, dtype=torch.int64)
    r = ref.sr_bits16(c, 0, 0)
    assert (r[0::2] != r[1::2]).double().mean().item() > 0.99
    assert 0 <= ref.sr_key(2 ** 63 + 5, 2 ** 40) < 2 ** 32


def test_fma32_is_correctly_rounded():
    """The oracle's fp32 fma against exact rational arithmetic, including sums
    that fp64 cannot hold exactly."""
    from fractions import Fraction

    g = torch.Generator().manual_seed(0)
    b = torch.randn(2000, generator=g)
    c = torch.randn(2000, generator=g) * (2.0 ** torch.randint(-40, 40, (2000,), generator=g).float())
    a = -1.2345e-4
    a32 = torch.tensor(a, dtype=torch.float32).item()
    got = ref._fma32(a, b, c)
    assert got.dtype == torch.float32
    below = torch.nextafter(got, torch.full_like(got, -math.inf))
    above = torch.nextafter(got, torch.full_like(got, math.inf))
    inexact_in_fp64 = 0
    for i in range(0, 2000, 3):
        exact = Fraction(a32) * Fraction(b[i].item()) + Fraction(c[i].item())
        inexact_in_fp64 += Fraction(a32 * b[i].item() + c[i].item()) != exact
        err = abs(Fraction(got[i].item()) - exact)  # no neighbouring fp32 is closer
        assert err <= abs(Fraction(below[i].item()) - exact) and err <= abs(Fraction(above[i].item()) - exact), i
    assert inexact_in_fp64 > 50


# --------------------------------------------------------- 3. unfreezing
def _run_constant_gradient(rounding, steps=2000, n=4096, start=1.0):
    p = torch.nn.Parameter(torch.full((n,), start, dtype=torch.bfloat16))
    opt = Lion([p], lr=1e-4, weight_decay=0.1, backend="torch", param_rounding=rounding, seed=11)
    p.grad = torch.ones(n, dtype=torch.bfloat16)
    for _ in range(steps):
        opt.step()
    return p.detach()


def test_stochastic_rounding_unfreezes_large_weights():
    steps, lr, wd = 2000, 1e-4, 0.1
    nearest = _run_constant_gradient("nearest", steps)
    assert torch.equal(nearest, torch.ones_like(nearest)), "round-to-nearest leaves 1.0 frozen: the defect"
    x = 1.0
    for _ in range(steps):  # the fp64 recurrence
        x = x * (1 - lr * wd) - lr
    assert abs(x - 0.78218) < 1e-5
    got = _run_constant_gradient("stochastic", steps).double()
    # per-step variance <= ulp^2 / 4 at the largest ulp visited (2^-8 below 1.0), a martingale sum over the
    # steps, averaged over 4096 coordinates; 6 sigma
    bound = 6 * math.sqrt(steps) * 2.0 ** -8 / 2 / math.sqrt(4096)
    print(f"stochastic mean {got.mean().item():.5f}  fp64 {x:.5f}  bound {bound:.2e}")
    assert abs(got.mean().item() - x) < bound
    assert got.std().item() > 0  # coordinates walk independently


# ------------------------------------------------------ 4. dtypes, values
def test_fp32_is_unaffected_fp16_and_bad_values_raise():
    torch.manual_seed(0)
    w = torch.randn(3000)
    outs = []
    for rounding in ("nearest", "stochastic"):
        p = torch.nn.Parameter(w.clone())
        opt = Lion([p], lr=1e-3, weight_decay=0.1, backend="torch", param_rounding=rounding)
        g = torch.Generator().manual_seed(1)
        for _ in range(3):
            p.grad = torch.randn(3000, generator=g)
            opt.step()
        assert opt.stats()["param_rounding"] == rounding
        outs.append(p.detach().clone())
    assert torch.equal(outs[0], outs[1])
    p = torch.nn.Parameter(w.clone().half())
    p.grad = torch.ones_like(p)
    with pytest.raises(ValueError, match="float16"):
        Lion([p], backend="torch", param_rounding="stochastic").step()
    Lion([p], backend="torch").step()  # nearest: fp16 still fine
    with pytest.raises(ValueError, match="param_rounding"):
        Lion([p], param_rounding="coin")
    with pytest.raises(TypeError):
        Lion([p], 1e-4, (0.9, 0.99), 0.0, None, "majority", "negative", "stochastic")  # keyword-only


# ------------------------------------------------------------- 5. gloo
def _model(seed=0):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Embedding(50, 12), torch.nn.Linear(12, 37), torch.nn.GELU(),
                              torch.nn.Linear(37, 50))
    return net.to(torch.bfloat16)


def _loss(net, x):
    logits = net(x).float()
    return torch.nn.functional.cross_entropy(logits.reshape(-1, 50), x.roll(1, 1).reshape(-1))


def _train(rank, world, exchange, vote, steps):
    from distributed_lion_pytorch_amd.optim.executors import coord_base

    lr, wd, seed = 1e-2, 0.1, 5
    net, oracle = _model(), _model()
    opt = Lion(net.parameters(), lr=lr, weight_decay=wd, exchange=exchange, vote=vote, bucket_mb=0.0005,
               param_rounding="stochastic", seed=seed)
    moms = {id(p): torch.zeros_like(p) for p in oracle.parameters()}
    nearest_differs = False
    for step in range(steps):
        x = torch.randint(0, 50, (4, 9), generator=torch.Generator().manual_seed(1000 * rank + step))
        opt.zero_grad()
        _loss(net, x).backward()
        opt.step()
        coords = {}
        for b in opt.plan.buckets:
            for s in b.segments:
                coords[s.index] = coord_base(b) + s.bit_off + torch.arange(s.numel, dtype=torch.int64)
        oracle.zero_grad()
        _loss(oracle, x).backward()
        with torch.no_grad():
            for i, p in enumerate(oracle.parameters()):
                m = moms[id(p)]
                bits = ref.sign_bits(p.grad, m, 0.9)
                allb = [torch.empty_like(bits) for _ in range(world)]
                dist.all_gather(allb, bits)
                delta = ref.vote_delta(torch.stack([b.reshape(-1) for b in allb]),
                                       torch.ones(world, dtype=torch.uint8), ref.VOTE_CODES[vote], ref.TIE_NEGATIVE)
                q = p.detach().clone()
                ref.apply_delta_(q, delta, lr, wd)
                ref.apply_delta_(p, delta, lr, wd, rounding=ref.ROUND_STOCHASTIC, coords=coords[i], seed=seed,
                                 step=step)
                nearest_differs |= not torch.equal(p, q)
                ref.momentum_update_(p.grad, m, 0.99)
    allc = torch.cat(list(coords.values()))
    return {"params": [p.detach().clone() for p in net.parameters()],
            "oracle_ok": all(torch.equal(a, b) for a, b in zip(net.parameters(), oracle.parameters())),
            "coords_unique": allc.unique().numel() == allc.numel(), "n_buckets": len(opt.plan.buckets),
            "nearest_differs": nearest_differs, "rounding": opt.stats()["param_rounding"]}


@pytest.mark.parametrize("world,exchange,vote", [(2, "a2a", "majority"), (2, "allgather", "majority"),
                                                 (3, "a2a", "majority"), (3, "allgather", "majority"),
                                                 (3, "a2a", "average"), (3, "allgather", "average")])
def test_gloo_replicas_identical_and_match_oracle(world, exchange, vote):
    res = run_world(_train, world, exchange, vote, 3)
    for r in res:
        assert r["oracle_ok"], "parameters differ from the single-process oracle with the same (seed, step)"
        assert r["coords_unique"] and r["n_buckets"] > 1
        assert r["nearest_differs"] and r["rounding"] == "stochastic"
        for a, b in zip(r["params"], res[0]["params"]):
            assert torch.equal(a, b), "replicas diverged"


# -------------------------------------------------------- 6. entrypoints
def _lion(trainer):
    opt = trainer.optimizer
    return getattr(opt, "optimizer", opt)


def test_entrypoint_flag_reaches_lion(tmp_path):
    import dpo_llama2
    import run_clm
    import sft_llama2

    flag = ["--lion_param_rounding", "stochastic"]
    tr = run_clm.main(["--synthetic_data", "--synthetic_samples", "16", "--block_size", "32",
                       "--per_device_train_batch_size", "2", "--learning_rate", "1e-3", "--report_to", "none",
                       "--use_cpu", "--config_name", "gpt2-tiny", "--max_steps", "1", "--lion", "--async_grad",
                       "--do_train", "--save_strategy", "no", "--output_dir", str(tmp_path / "clm")] + flag)
    assert _lion(tr).param_rounding == "stochastic" and _lion(tr).stats()["steps"] == 1
    tr = sft_llama2.main(["--model_name", "llama-tiny", "--synthetic_data", "--synthetic_samples", "40", "--seq_length",
                          "32", "--output_dir", str(tmp_path / "sft"), "--max_steps", "1",
                          "--per_device_train_batch_size", "2", "--learning_rate", "1e-3", "--lion", "--async_grad",
                          "--report_to", "none", "--use_cpu", "--torch_dtype", "float32"] + flag)
    assert _lion(tr).param_rounding == "stochastic"
    tr = dpo_llama2.main(["--model_name_or_path", "llama-tiny", "--synthetic_data", "--synthetic_samples", "60",
                          "--max_length", "1024", "--max_prompt_length", "256", "--output_dir", str(tmp_path / "dpo"),
                          "--max_steps", "1", "--per_device_train_batch_size", "2", "--gradient_accumulation_steps",
                          "1", "--lion", "--async_grad", "--use_cpu", "--torch_dtype", "float32", "--eval_steps", "0",
                          "--warmup_steps", "1", "--final_save", "false"] + flag)
    assert _lion(tr).param_rounding == "stochastic"
    # the default is the reference's rounding
    from distributed_lion_pytorch_amd.trainer.async_trainer import LionArguments

    assert LionArguments().lion_param_rounding == "nearest"


# ----------------------------------------------------- 7. register budget
CSRC = Path(ROOT) / "distributed_lion_pytorch_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
def test_lion_kernels_do_not_spill(tmp_path):
    """No ``lion_*`` kernel, the stochastic-rounding instantiations included,
    reports a VGPR or SGPR spill (the compile of tests/test_kernel_resources_cpu.py).

    The majority pair kernel ``lion_apply_pair_kernel<DT, true, 2>`` used to
    spill 70 (bf16), 96 (fp32) and 82 (fp16) SGPRs into VGPR lanes: hoisted
    64-bit lane masks of the uniform "plane k is live" tests.  ``vote_word``
    now tests a per-call copy of the live mask (docs/DESIGN.md, "Stochastic
    rounding of the parameter store")."""
    src = "lion_kernels.hip"
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", f"-I{CSRC}", "-c", str(CSRC / src),
           "-o", str(tmp_path / (src + ".o")), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark: *(VGPRs Spill|SGPRs Spill): (\d+)", line)
        if m and name:
            res[name][m.group(1)] = int(m.group(2))
    lion = {k: v for k, v in res.items() if re.search(r"\d+lion_\w+_kernel", k)}
    # K0, byte K2, sliced K2, pair (pre-voted, majority), counted (plain, telemetry): 7 stochastic instantiations
    sr = [k for k in lion if re.search(r"Lb1EEEv", k) and "lion_encode" not in k]
    assert len(sr) == 7, sorted(lion)
    assert all(len(v) == 2 for v in lion.values()), "the remarks changed format"
    spilled = {k: v for k, v in lion.items() if v["VGPRs Spill"] or v["SGPRs Spill"]}
    assert not spilled, f"register spills in {src}: {spilled}"
