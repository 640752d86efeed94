#!/usr/bin/env python
"""Record what the reference optimizer computes, as fixtures under tests/golden/.

The parity tests (tests/test_oracle.py, tests/test_distributed_cpu.py) compare
this project's Lion with the reference implementation bit for bit.  So that
they need no copy of the reference at test time, this tool runs the reference
once on fixed inputs and stores inputs and results:

  lion_reference_update_fn.pt   update_fn on single tensors (fp32, bf16)
  lion_reference_single.pt      4 single-process optimizer steps of a small net
  lion_reference_w2.pt / _w3.pt 3 distributed steps on 2 / 3 gloo ranks

Every file holds the initial weights, the gradients fed to the optimizer at
each step (per rank) and the parameters / momenta the reference produced, so a
test replays the gradients through this project's optimizer and compares.

  python tools/make_reference_golden.py --reference PATH/TO/distributed_lion.py
"""
import argparse
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_reference(path):
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("_ref_distributed_lion", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _clone(ts):
    return [t.detach().clone() for t in ts]


def record_update_fn(R):
    cases = []
    for dtype in (torch.float32, torch.bfloat16):
        g = torch.Generator().manual_seed(0)
        for shape in [(7,), (33, 17), (768,)]:
            p0 = torch.randn(shape, generator=g).to(dtype)
            gr = torch.randn(shape, generator=g).to(dtype)
            m0 = torch.randn(shape, generator=g).to(dtype) * 0.1
            p, m = p0.clone(), m0.clone()
            R.update_fn(p, gr, m, 1e-3, 0.1, 0.9, 0.99)
            cases.append({"p0": p0, "grad": gr, "m0": m0, "p": p, "m": m})
    return {"hyper": {"lr": 1e-3, "wd": 0.1, "beta1": 0.9, "beta2": 0.99}, "cases": cases}


def record_single(R):
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(20, 31), torch.nn.Tanh(), torch.nn.Linear(31, 5)).bfloat16()
    init = {k: v.clone() for k, v in net.state_dict().items()}
    opt = R.Lion(net.parameters(), lr=3e-3, weight_decay=0.05)
    grads, params = [], []
    for _ in range(4):
        x = torch.randn(8, 20).bfloat16()
        opt.zero_grad()
        net(x).float().pow(2).mean().backward()
        grads.append(_clone(p.grad for p in net.parameters()))
        opt.step()
        params.append(_clone(net.parameters()))
    sd = opt.state_dict()
    return {"init": init, "grads": grads, "params": params,
            "exp_avg": [sd["state"][k]["exp_avg"].clone() for k in sorted(sd["state"])],
            "state_keys": sorted({kk for k in sd["state"] for kk in sd["state"][k]}),
            "param_group_keys": sorted(sd["param_groups"][0].keys())}


def _record_rank(rank, world, ref_path):
    from test_distributed_cpu import _batch, _loss, _model

    R = load_reference(ref_path)
    net = _model(3)
    init = {k: v.clone() for k, v in net.state_dict().items()}
    opt = R.Lion(net.parameters(), lr=2.0 ** -7, weight_decay=0.1)
    grads, params = [], []
    for step in range(3):
        opt.zero_grad()
        _loss(net, _batch(rank, step)).backward()
        grads.append(_clone(p.grad for p in net.parameters()))
        opt.step()
        params.append(_clone(net.parameters()))
    return {"init": init, "grads": grads, "params": params,
            "exp_avg": _clone(opt.state[p]["exp_avg"] for p in net.parameters())}


def record_distributed(ref_path, world):
    from dist_utils import run_world

    res = run_world(_record_rank, world, ref_path)
    for r in res[1:]:  # the vote keeps the replicas identical
        assert all(torch.equal(a, b) for sa, sb in zip(r["params"], res[0]["params"]) for a, b in zip(sa, sb))
    return {"world": world, "lr": 2.0 ** -7, "weight_decay": 0.1, "init": res[0]["init"],
            "grads": [r["grads"] for r in res], "params": res[0]["params"], "exp_avg": [r["exp_avg"] for r in res]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="path of the reference's distributed_lion.py")
    a = ap.parse_args()
    torch.set_num_threads(1)
    R = load_reference(a.reference)
    os.makedirs(GOLDEN, exist_ok=True)
    torch.save(record_update_fn(R), os.path.join(GOLDEN, "lion_reference_update_fn.pt"))
    torch.save(record_single(R), os.path.join(GOLDEN, "lion_reference_single.pt"))
    for world in (2, 3):
        torch.save(record_distributed(os.path.abspath(a.reference), world),
                   os.path.join(GOLDEN, f"lion_reference_w{world}.pt"))


if __name__ == "__main__":
    main()
