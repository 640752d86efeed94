"""Average voting over the all-to-all exchange end to end on the GPU: two gloo
ranks on ONE GPU (HIP kernels: encode, K4c shard count, counted apply) against
the all-gather exchange's average (the byte kernel), and the same path over a
1-rank RCCL group in a fresh interpreter."""
import json
import os
import subprocess
import sys
import textwrap

import pytest
import torch

from dist_utils import free_port, run_world

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEPS = 3

PRELUDE = textwrap.dedent("""
    import json, os, sys
    import torch, torch.distributed as dist
    sys.path.insert(0, sys.argv[1])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    assert dist.get_backend() == "nccl"
    out = {}
""")
EPILOGUE = textwrap.dedent("""
    torch.cuda.synchronize()
    dist.destroy_process_group()
    print("RESULT " + json.dumps(out), flush=True)
""")


def _run(body: str, timeout: int = 150) -> dict:
    """A 1-rank ``nccl`` scenario in a fresh interpreter (a process group per process)."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()),
               RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    code = PRELUDE + textwrap.dedent(body) + EPILOGUE
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=timeout, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
    assert line, r.stdout[-2000:]
    return json.loads(line[-1][len("RESULT "):])


def _train(rank, world, exchange, force_counts):
    import torch.distributed as dist

    from distributed_lion_pytorch_amd import Lion
    from distributed_lion_pytorch_amd.models.gpt2 import GPT2LMHeadModel, gpt2_config
    from distributed_lion_pytorch_amd.trainer.engine import TrainStep

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = gpt2_config("gpt2-tiny")
    torch.manual_seed(0)
    model = GPT2LMHeadModel(cfg).to(device=dev, dtype=torch.bfloat16)
    opt = Lion(model.parameters(), lr=1e-3, weight_decay=0.1, exchange=exchange, vote="average", backend="hip",
               telemetry=True)
    opt._force_counts = force_counts
    step = TrainStep(model, opt, grad_accum=2)
    gen = torch.Generator(device=dev).manual_seed(100 + rank)

    def batches():
        for _ in range(2):
            ids = torch.randint(0, cfg.vocab_size, (2, 64), device=dev, generator=gen)
            yield {"input_ids": ids, "labels": ids}

    for _ in range(STEPS):
        step(batches())
    torch.cuda.synchronize()
    flat = torch.cat([p.detach().float().reshape(-1) for p in model.parameters()]).cpu()
    digest = torch.tensor([flat.double().sum().item(), (flat.double() ** 2).sum().item()])
    others = [torch.empty_like(digest) for _ in range(world)]
    dist.all_gather(others, digest)
    return {"flat": flat, "digests": [o.tolist() for o in others], "executor": type(opt._executor).__name__,
            "stats": opt.stats(), "plan_bytes": opt.plan.total_bytes}


def test_two_ranks_one_gpu_counts_equal_allgather_average():
    world = 2
    cnt = run_world(_train, world, "a2a", True)
    ag = run_world(_train, world, "allgather", False)
    for r in cnt + ag:
        assert r["executor"] == "HipExecutor"
        assert r["digests"][0] == r["digests"][1], "replicas diverged"
    assert all(r["stats"]["exchange_impl"] == "AllToAllExchange+counts" for r in cnt)
    assert all(r["stats"]["exchange_impl"] == "AllGatherExchange" for r in ag)
    assert torch.equal(cnt[0]["flat"], cnt[1]["flat"])
    assert torch.equal(ag[0]["flat"], ag[1]["flat"])
    assert torch.equal(cnt[0]["flat"], ag[0]["flat"])
    # measured receive bytes per step: (W-1)/W * (1+P) planes of the plan's bytes
    p = world.bit_length()
    for r in cnt:
        assert r["stats"]["wire_bytes_recv"] == STEPS * (world - 1) * (1 + p) * r["plan_bytes"] // world
        assert r["stats"]["vote_agree"] > 0
    for r in ag:
        assert r["stats"]["wire_bytes_recv"] == STEPS * (world - 1) * r["plan_bytes"]
    # the same votes: the same agreement count on both paths
    assert cnt[0]["stats"]["vote_agree"] == ag[0]["stats"]["vote_agree"]


def test_counts_over_rccl_one_rank_equals_allgather_average():
    out = _run("""
        from distributed_lion_pytorch_amd import Lion
        from distributed_lion_pytorch_amd.models.gpt2 import GPT2LMHeadModel, gpt2_config
        res = {}
        for name, exchange, counts in (("counts", "a2a", True), ("allgather", "allgather", False)):
            torch.manual_seed(0)
            cfg = gpt2_config("gpt2-tiny")
            model = GPT2LMHeadModel(cfg).to(device=dev, dtype=torch.bfloat16)
            opt = Lion(model.parameters(), lr=1e-3, weight_decay=0.1, exchange=exchange, vote="average",
                       backend="hip", bucket_mb=0.004)
            opt._force_vote = True
            opt._force_counts = counts
            g = torch.Generator(device=dev).manual_seed(3)
            for _ in range(3):
                ids = torch.randint(0, cfg.vocab_size, (2, 64), device=dev, generator=g)
                model(ids, labels=ids)["loss"].backward()
                opt.step()
                opt.zero_grad()
            torch.cuda.synchronize()
            res[name] = torch.cat([p.detach().float().reshape(-1) for p in model.parameters()])
            st = opt.stats()
            out[name + "_impl"] = st["exchange_impl"]
            out[name + "_collectives"] = st["collectives"]
            out[name + "_executor"] = st["executor"]
        out["equal"] = torch.equal(res["counts"], res["allgather"])
        out["n_buckets"] = len(opt.plan.buckets)
    """)
    assert out["equal"], out
    assert out["counts_impl"] == "AllToAllExchange+counts" and out["allgather_impl"] == "AllGatherExchange"
    assert out["counts_executor"] == out["allgather_executor"] == "HipExecutor"
    assert out["n_buckets"] > 1
    assert out["counts_collectives"] == 3 * 2 * out["n_buckets"]  # all-to-all + ONE all-gather per bucket
