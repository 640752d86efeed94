"""Stochastic rounding of the bf16 parameter store on the gfx950 kernels: every
kernel that stores parameters (K0 and all K2 routes), bit for bit against the
PyTorch-oracle executor with the same (seed, step), over several buckets and
coordinate bases; non-degeneracy; fp32; the optimizer; two ranks on one GPU."""
import copy

import pytest
import torch

from dist_utils import run_world
from distributed_lion_pytorch_amd.ops import hip
from distributed_lion_pytorch_amd.ops import reference as ref
from distributed_lion_pytorch_amd.optim.executors import HParams, HipExecutor, TorchExecutor
from distributed_lion_pytorch_amd.optim.plan import FlatPlan

pytestmark = pytest.mark.gpu

# the kernel tests' sizes (tail paths, one element past a 2048 / 8192 boundary, an odd large tensor) plus one
# full chunk and five full chunks: the vectorised full-chunk paths and the full chunk pairs of the pair kernels
SIZES = [1, 7, 8, 13, 2047, 2048, 2049, 8192, 8193, 40_960, 300_001]
SR = dict(rounding=ref.ROUND_STOCHASTIC, seed=7, step=3)
HP = HParams(lr=3e-3, wd=0.05, beta1=0.9, beta2=0.99)


@pytest.fixture(autouse=True)
def _need_hip(cuda):
    hip.require()


def _tensors(dtype, dev, seed=0, sizes=SIZES):
    g = torch.Generator(device="cpu").manual_seed(seed)
    ps, gs, ms = [], [], []
    for i, n in enumerate(sizes):
        p = torch.randn(n, generator=g).to(dtype)
        gr = torch.randn(n, generator=g).to(dtype)
        m = (torch.randn(n, generator=g) * 0.5).to(dtype)
        if i == 5:  # storage offset by one element: not 16-B aligned
            p = torch.cat([p.new_zeros(1), p])[1:]
        ps.append(p.to(dev))
        gs.append(gr.to(dev))
        ms.append(m.to(dev))
    return ps, gs, ms


def _clone(ts):
    return [t.clone() for t in ts]


def _rebind(bucket, new_params, byte_shift=0):
    """The bucket over other parameter tensors, optionally moved up in the
    plan's byte space (a coordinate base past 2^32 without a 1 GB plan)."""
    b2 = copy.copy(bucket)
    b2.byte_off = bucket.byte_off + byte_shift
    b2.segments = [copy.copy(s) for s in bucket.segments]
    for s in b2.segments:
        s.param = new_params[s.index]
    return b2


def _equal(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), (i, a.numel(), (a != b).sum().item())


# ------------------------------------------------------------------ 1. K0
@pytest.mark.parametrize("byte_shift", [0, 1 << 33])
def test_local_stochastic_matches_oracle(byte_shift, cuda):
    ps, gs, ms = _tensors(torch.bfloat16, cuda)
    plan = FlatPlan([(p, 0) for p in ps], world=1, bucket_bytes=1 << 12, device=cuda)
    assert len(plan.buckets) > 2
    p2, m2 = _clone(ps), _clone(ms)
    hx, tx = HipExecutor(plan), TorchExecutor(plan)
    meta = plan.meta(gs, ms)
    for b in plan.buckets:
        hx.local(meta, _rebind(b, ps, byte_shift), HP, **SR)
        tx.local(None, _rebind(b, p2, byte_shift), HP, grads=gs, moms=m2, **SR)
    torch.cuda.synchronize()
    _equal(ps, p2)
    _equal(ms, m2)


# ------------------------------------------------------- 2. every K2 route
def _count_planes(hx, plan, planes, alive, world, dev):
    """[W][P][shard] count planes of every bucket, as the a2a exchange gathers them."""
    npl = world.bit_length()
    counts = torch.zeros(npl * plan.total_bytes, dtype=torch.uint8, device=dev)
    for b in plan.buckets:
        sh = b.nbytes // world
        pl = planes[world * b.byte_off: world * (b.byte_off + b.nbytes)].view(world, b.nbytes)
        for r in range(world):
            o = npl * b.byte_off + r * npl * sh
            hx.vote_count(pl[:, r * sh:(r + 1) * sh].contiguous().view(-1), sh, alive, counts[o:o + npl * sh])
    return counts


ROUTES = [
    # id, mode, world, negative plane, telemetry            -> kernel
    ("prevoted", ref.VOTE_PREVOTED, 4, False, False),       # pair kernel, pre-voted
    ("prevoted_neg", ref.VOTE_PREVOTED, 4, True, False),
    ("majority_w3", ref.VOTE_MAJORITY, 3, False, False),    # pair kernel, majority
    ("majority_w8", ref.VOTE_MAJORITY, 8, False, False),
    ("prevoted_neg_tel", ref.VOTE_PREVOTED, 4, True, True),  # telemetry: the sliced one-chunk kernel
    ("majority_w3_tel", ref.VOTE_MAJORITY, 3, False, True),
    ("average_w4", ref.VOTE_AVERAGE, 4, False, False),      # byte kernel
    ("average_w4_tel", ref.VOTE_AVERAGE, 4, False, True),
    ("majority_w16", ref.VOTE_MAJORITY, 16, False, True),   # byte kernel (W > 15)
    ("counted_w5", ref.VOTE_COUNTED, 5, False, False),      # counted, two chunks per block
    ("counted_w5_tel", ref.VOTE_COUNTED, 5, False, True),   # counted, telemetry
]


@pytest.mark.parametrize("name,mode,world,with_neg,tel", ROUTES, ids=[r[0] for r in ROUTES])
def test_apply_routes_stochastic_match_oracle(name, mode, world, with_neg, tel, cuda):
    ps, gs, ms = _tensors(torch.bfloat16, cuda, seed=2)
    plan = FlatPlan([(p, 0) for p in ps], world=world, bucket_bytes=1 << 12, device=cuda)
    assert len(plan.buckets) > 2
    gen = torch.Generator(device="cpu").manual_seed(world)
    planes = torch.randint(0, 256, (world * plan.total_bytes,), generator=gen, dtype=torch.uint8).to(cuda)
    own_all = torch.randint(0, 256, (plan.total_bytes,), generator=gen, dtype=torch.uint8).to(cuda)
    alive = torch.ones(world, dtype=torch.uint8, device=cuda)
    if world > 2 and mode != ref.VOTE_PREVOTED:
        alive[1] = 0
    tie = ref.TIE_ZERO if with_neg else ref.TIE_NEGATIVE
    hx, tx = HipExecutor(plan), TorchExecutor(plan)
    meta = plan.meta(gs, ms)
    if mode == ref.VOTE_COUNTED:
        counts = _count_planes(hx, plan, planes, alive, world, cuda)
        npl = world.bit_length()
    p2 = _clone(ps)
    agree = torch.zeros(2, dtype=torch.int64, device=cuda)
    agree_t = torch.zeros(2, dtype=torch.int64, device=cuda)
    for b in plan.buckets:
        sl = slice(b.byte_off, b.byte_off + b.nbytes)
        neg = None
        if mode == ref.VOTE_PREVOTED:
            pl, stride = planes[sl], b.nbytes
            if with_neg:
                neg = planes[plan.total_bytes:][sl] & ~pl
        elif mode == ref.VOTE_COUNTED:
            pl, stride = counts[npl * b.byte_off: npl * (b.byte_off + b.nbytes)], b.nbytes // world
        else:
            pl, stride = planes[world * b.byte_off: world * (b.byte_off + b.nbytes)], b.nbytes
        kw = dict(own=own_all[sl], agree=agree) if tel else {}
        kw_t = dict(own=own_all[sl], agree=agree_t) if tel else {}
        hx.apply(meta, b, pl, stride, alive, mode, tie, neg, HP, **kw, **SR)
        tx.apply(None, _rebind(b, p2), pl, stride, alive, mode, tie, neg, HP, **kw_t, **SR)
    torch.cuda.synchronize()
    _equal(ps, p2)
    if tel:
        assert agree[0].item() == agree_t[0].item() > 0
        if mode not in (ref.VOTE_PREVOTED, ref.VOTE_COUNTED):  # (those count their ties in the shard vote)
            assert agree[1].item() == agree_t[1].item()


# --------------------------------------------------------- 3. non-degeneracy
def test_streams_differ_by_step_and_repeat_exactly(cuda):
    ps, gs, ms = _tensors(torch.bfloat16, cuda, seed=4)
    # lr / ulp is fractional for every |p| of a randn tensor: 0.13 in [1, 2), 0.26 in [0.5, 1), 0.51 in
    # [0.25, 0.5), ...; a store differs from nearest with probability min(f, 1 - f) of that fraction f: > 10 %
    hp = HParams(lr=1e-3, wd=0.1, beta1=0.9, beta2=0.99)

    def run_on_clone(**kw):  # a plan of its own: the kernels' pointer table names the cloned tensors
        p2, m2 = _clone(ps), _clone(ms)
        plan = FlatPlan([(p, 0) for p in p2], world=1, bucket_bytes=1 << 12, device=cuda)
        hx = HipExecutor(plan)
        meta = plan.meta(gs, m2)
        for b in plan.buckets:
            hx.local(meta, b, hp, **kw)
        torch.cuda.synchronize()
        return torch.cat([p.reshape(-1) for p in p2])

    a = run_on_clone(rounding=ref.ROUND_STOCHASTIC, seed=1, step=5)
    a2 = run_on_clone(rounding=ref.ROUND_STOCHASTIC, seed=1, step=5)
    b = run_on_clone(rounding=ref.ROUND_STOCHASTIC, seed=1, step=6)
    near = run_on_clone()
    assert torch.equal(a, a2)
    assert not torch.equal(a, b)
    assert (a != near).float().mean().item() >= 0.10
    # a stochastic store is a bf16 neighbour of x = fma(-lr, s, p * decay): |a - x| < ulp(x).  Nearest stores
    # rne(y), y = rne(p * decay) - lr * s, with |y - x| <= half an ulp of p <= |p| 2^-8 and |rne(y) - y| <= half
    # an ulp of y; an ulp of v is at most |v| 2^-7
    p0 = torch.cat([p.reshape(-1) for p in ps]).float().abs()
    big = torch.maximum(a.float().abs(), near.float().abs())
    assert bool(((a.float() - near.float()).abs() <= 1.5 * big * 2.0 ** -7 + p0 * 2.0 ** -8).all())


# ------------------------------------------------------------------ 4. fp32
def test_fp32_stochastic_equals_nearest(cuda):
    outs = []
    for kw in ({}, SR):
        ps, gs, ms = _tensors(torch.float32, cuda, seed=5)
        plan = FlatPlan([(p, 0) for p in ps], world=4, bucket_bytes=1 << 12, device=cuda)
        hx = HipExecutor(plan)
        meta = plan.meta(gs, ms)
        pos = torch.randint(0, 256, (plan.total_bytes,), generator=torch.Generator().manual_seed(1),
                            dtype=torch.uint8).to(cuda)
        alive = torch.ones(4, dtype=torch.uint8, device=cuda)
        for b in plan.buckets:
            hx.local(meta, b, HP, **kw)
            hx.apply(meta, b, pos[b.byte_off:b.byte_off + b.nbytes], b.nbytes, alive, ref.VOTE_PREVOTED,
                     ref.TIE_NEGATIVE, None, HP, **kw)
        torch.cuda.synchronize()
        outs.append(ps + ms)
    _equal(outs[0], outs[1])


def test_fp16_is_refused_by_the_op(cuda):
    ps, gs, ms = _tensors(torch.float16, cuda, seed=6, sizes=[2048])
    plan = FlatPlan([(p, 0) for p in ps], world=1, device=cuda)
    with pytest.raises(RuntimeError, match="fp16"):
        HipExecutor(plan).local(plan.meta(gs, ms), plan.buckets[0], HP, **SR)


# ------------------------------------------------------------- 5. optimizer
def _mlp():
    return torch.nn.Sequential(torch.nn.Linear(64, 257), torch.nn.GELU(), torch.nn.Linear(257, 64)).bfloat16()


def test_lion_stochastic_gpu_single_rank_matches_torch_backend(cuda):
    """Lion on the kernels against Lion(backend="torch"), both over GPU tensors
    as in test_kernels_gpu's optimizer test: the momentum and the sign are the
    nearest path's ATen-HIP arithmetic (fma with an fp32 alpha).  ATen on the
    CPU rounds the bf16 axpy's alpha to bf16 first, so a CPU run of the oracle
    differs from any GPU run in the momentum -- with either rounding mode."""
    from distributed_lion_pytorch_amd import Lion

    torch.manual_seed(0)
    net, net_ref = _mlp(), _mlp()
    net_ref.load_state_dict(net.state_dict())
    net, net_ref = net.to(cuda), net_ref.to(cuda)
    kw = dict(lr=1e-3, weight_decay=0.1, param_rounding="stochastic", seed=9, bucket_mb=0.002)
    opt, opt_ref = Lion(net.parameters(), **kw), Lion(net_ref.parameters(), backend="torch", **kw)
    for step in range(3):
        grads = [torch.randn(p.shape, generator=torch.Generator().manual_seed(10 * step + i)).bfloat16()
                 for i, p in enumerate(net_ref.parameters())]
        for p, q, g in zip(net.parameters(), net_ref.parameters(), grads):
            p.grad, q.grad = g.to(cuda), g.to(cuda)
        opt.step()
        opt_ref.step()
    assert type(opt._executor).__name__ == "HipExecutor" and type(opt_ref._executor).__name__ == "TorchExecutor"
    assert opt.stats()["param_rounding"] == "stochastic" and len(opt.plan.buckets) > 1
    for a, b in zip(net.parameters(), net_ref.parameters()):
        assert torch.equal(a, b)
        assert torch.equal(opt.state[a]["exp_avg"], opt_ref.state[b]["exp_avg"])


# ------------------------------------------------------------ 6. two ranks
def _train(rank, world, exchange, steps):
    from distributed_lion_pytorch_amd import Lion

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    nets = [_mlp().to(dev) for _ in range(2)]
    nets[1].load_state_dict(nets[0].state_dict())
    kw = dict(lr=1e-3, weight_decay=0.1, exchange=exchange, param_rounding="stochastic", seed=3, bucket_mb=0.002)
    opts = [Lion(nets[0].parameters(), backend="hip", **kw), Lion(nets[1].parameters(), backend="torch", **kw)]
    for step in range(steps):
        for net, opt in zip(nets, opts):
            for i, p in enumerate(net.parameters()):
                g = torch.Generator().manual_seed(1000 * rank + 10 * step + i)
                p.grad = torch.randn(p.shape, generator=g).bfloat16().to(dev)
            opt.step()
    torch.cuda.synchronize()
    flat = [torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu() for net in nets]
    return {"hip": flat[0], "torch": flat[1], "executor": type(opts[0]._executor).__name__}


def test_two_ranks_one_gpu_stochastic_replicas_identical():
    res = run_world(_train, 2, "a2a", 3)
    assert res[0]["executor"] == "HipExecutor"
    assert torch.equal(res[0]["hip"], res[1]["hip"]), "replicas diverged"
    assert torch.equal(res[0]["hip"], res[0]["torch"]), "HIP kernels differ from the oracle executor"
