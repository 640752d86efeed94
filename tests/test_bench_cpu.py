"""bench.py launch contract on the CPU: ``--gpus N`` without torchrun starts N
real ranks (never a silent dp1), a WORLD_SIZE that disagrees with ``--gpus``
or too few devices is a hard error, and the JSON carries the measured wire
bytes and the per-phase breakdown of the step."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--model", "gpt2-tiny", "--micro_batch", "2", "--grad_accum", "2", "--seq_len", "64", "--steps", "2",
        "--warmup", "1"]


def _run(args, env=None, timeout=300):
    e = dict(os.environ, OMP_NUM_THREADS="2")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, capture_output=True, text=True,
                          timeout=timeout, env=e)


def test_gpus3_without_torchrun_spawns_three_ranks():
    r = _run(["--gpus", "3", "--backend", "gloo", "--device", "cpu"] + TINY)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 only
    out = lines[0]
    assert out["n_gpus"] == 3 and out["config"]["parallelism"] == "dp3"
    assert out["launcher"] == "bench.py" and len(out["ms_per_step_per_rank"]) == 3
    meas = out["wire_bytes_per_step_per_rank_measured"]
    assert meas["wire_bytes_sent"] > 0 and meas["wire_bytes_recv"] > 0 and meas["collectives"] == 2  # a2a + AG
    assert out["wire_bytes_per_step_per_rank"] == meas["wire_bytes_sent"]
    # 1-bit vote-RS/AG: 2(W-1)/W * N/8 analytic, measured adds only the 256*W-byte bucket padding
    assert out["wire_bytes_per_step_per_rank_analytic"] <= meas["wire_bytes_sent"] < 2 * out[
        "wire_bytes_per_step_per_rank_analytic"]
    ph = out["phase_ms_per_step"]
    assert {"fwd_bwd", "clip", "optimizer", "encode", "exchange", "apply"} <= set(ph)
    assert all(v >= 0 for v in ph.values())
    assert ph["optimizer"] >= ph["encode"] and out["ms_per_step"] >= ph["fwd_bwd"]
    assert abs(out["value"] - 3 * 2 * 2 * 64 * 2 / (out["ms_per_step"] * 2 / 1000)) / out["value"] < 0.01


def test_dump_outputs_repeatable_and_full_accepted(tmp_path):
    """``--dump-outputs DIR`` writes the last timed step's loss and the sampled
    parameters / momenta as float32 .npy files; the same arguments give the
    same inputs and so (on the CPU, bit for bit) the same outputs.  ``--full``
    is accepted and reports the same fields."""
    import numpy as np

    dumps = []
    for tag, extra in (("a", ["--full"]), ("b", [])):
        d = tmp_path / tag
        r = _run(["--gpus", "1", "--device", "cpu", "--dump-outputs", str(d)] + extra + TINY)
        assert r.returncode == 0, r.stderr[-3000:]
        out = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
        assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["unit"] == "tokens/s"
        arrs = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
        assert set(arrs) == {"loss", "params", "exp_avg"}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
        assert arrs["loss"].shape == (1,) and abs(float(arrs["loss"][0]) - out["loss"]) < 1e-3
        assert arrs["params"].size == arrs["exp_avg"].size > 0 and np.abs(arrs["exp_avg"]).max() > 0
        assert sum(a.nbytes for a in arrs.values()) <= 64 * 2**20
        dumps.append(arrs)
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k


def test_dump_sample_is_fixed_and_bounded():
    """Outputs larger than the budget are sampled: the same elements every
    time, every tensor represented, within the budget plus the per-tensor floor."""
    sys.path.insert(0, ROOT)
    import bench

    ts = [torch.arange(50000, dtype=torch.bfloat16), torch.arange(100.0), torch.arange(3000.0).view(30, 100)]
    a = bench._sample_flat(ts, budget=10000)
    b = bench._sample_flat(ts, budget=10000)
    assert a.dtype.name == "float32" and (a == b).all()
    assert 100 + 1024 < a.size <= 10000 + 3 * 1024
    assert (a[-1024:] < 3000).all() and (a[-1124:-1024] == torch.arange(100.0).numpy()).all()
    full = bench._sample_flat(ts, budget=10**6)
    assert full.size == 53100


def test_world_size_mismatch_is_an_error():
    r = _run(["--gpus", "2", "--device", "cpu", "--backend", "gloo"] + TINY,
             env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in r.stderr


@pytest.mark.skipif(torch.cuda.device_count() >= 2, reason="needs a host with fewer than 2 GPUs")
def test_too_few_gpus_is_an_error():
    r = _run(["--gpus", "2", "--device", "cuda"] + TINY)
    assert r.returncode != 0
    assert "GPU(s) visible" in r.stderr


def test_learning_curves_native_vs_reference_track(tmp_path):
    """bench.py learning-curve mode on the learnable Markov corpus: the native
    engine and the reference algorithm (HF model + per-tensor int64 all_gather
    Lion) start from the same weights and their losses track step by step."""
    curves = {}
    for impl in ("native", "reference"):
        log = str(tmp_path / f"{impl}.jsonl")
        r = _run(["--device", "cpu", "--model", "gpt2-tiny", "--micro_batch", "4", "--grad_accum", "2", "--seq_len",
                  "64", "--steps", "20", "--data", "markov", "--loss_log", log, "--lr", "1e-3", "--impl", impl])
        assert r.returncode == 0, r.stderr[-3000:]
        curves[impl] = [json.loads(x)["loss"] for x in open(log)]
    a, b = curves["native"], curves["reference"]
    assert len(a) == len(b) == 20
    assert a[-1] < a[0] - 0.5  # it learns
    assert max(abs(x - y) for x, y in zip(a, b)) < 0.05


def test_reference_model_keeps_hf_default_attention():
    """The reference run's HF model uses HF's default SDPA attention, as the
    reference's run_clm does: building the native init weights (same seed) must
    not flip the shared config to the eager path (that cost the reference run
    30 % on the GPU: 331k -> 229k tok/s, profiles/r3/reference_sdpa.txt)."""
    import argparse

    sys.path.insert(0, ROOT)
    import bench

    args = argparse.Namespace(model="gpt2-tiny", dropout=None, lr=1e-4, weight_decay=0.1)
    model, _, cfg = bench.build_reference(args, torch.device("cpu"))
    assert model.config._attn_implementation == "sdpa"


def test_kfd_topology_gpu_count(tmp_path, monkeypatch):
    """The HIP-free GPU count's sysfs path: CPU nodes (simd_count 0) are not
    GPUs; a visibility variable caps the count."""
    from distributed_lion_pytorch_amd.utils import devices

    for i, simds in enumerate([0, 1024, 1024, 0]):
        d = tmp_path / str(i)
        d.mkdir()
        (d / "properties").write_text(f"cpu_cores_count 0\nsimd_count {simds}\nmax_waves_per_simd 8\n")
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(var, raising=False)
    assert devices._kfd_count(str(tmp_path)) == 2
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "1")
    assert devices._kfd_count(str(tmp_path)) == 1
    assert devices._kfd_count(str(tmp_path / "missing")) is None
