"""Average voting over the all-to-all exchange (count bit planes), CPU / gloo:
the torch executor's K4c + counted apply against the per-tensor oracle, the
W >= 5 routing rule, the measured wire bytes against the analytic formula,
simulated dropout against the all-gather exchange."""
import pytest
import torch
import torch.distributed as dist

from dist_utils import run_world

LR, WD = 2.0 ** -6, 0.1  # lr exactly representable in bf16 (CPU ATen rounds alpha to the tensor dtype)


def _model(seed=0, dtype=torch.bfloat16):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Embedding(40, 10), torch.nn.Linear(10, 300), torch.nn.Tanh(),
                              torch.nn.Linear(300, 40))
    return net.to(dtype)


def _batch(rank, step):
    g = torch.Generator().manual_seed(977 * rank + step)
    return torch.randint(0, 40, (3, 7), generator=g)


def _loss(net, x):
    return torch.nn.functional.cross_entropy(net(x).float().reshape(-1, 40), x.roll(1, 1).reshape(-1))


def _flat(net):
    return torch.cat([p.detach().float().reshape(-1) for p in net.parameters()])


def _train(rank, world, exchange, force_counts, steps, dropout):
    """Lion(vote='average') against the per-tensor oracle (all ranks alive) --
    or, with a dropout schedule, just the final parameters."""
    from distributed_lion_pytorch_amd import Lion
    from distributed_lion_pytorch_amd.ops import reference as ref

    net, oracle = _model(), _model()
    opt = Lion(net.parameters(), lr=LR, weight_decay=WD, exchange=exchange, vote="average", bucket_mb=0.0005,
               telemetry=True)
    opt._force_counts = force_counts
    if dropout:
        opt.set_dropout_schedule(dropout)
    moms = {id(p): torch.zeros_like(p) for p in oracle.parameters()}
    for step in range(steps):
        x = _batch(rank, step)
        opt.zero_grad()
        _loss(net, x).backward()
        opt.step()
        if dropout:
            continue
        oracle.zero_grad()
        _loss(oracle, x).backward()
        with torch.no_grad():
            for p in oracle.parameters():
                m = moms[id(p)]
                bits = ref.sign_bits(p.grad, m, 0.9)
                allb = [torch.empty_like(bits) for _ in range(world)]
                dist.all_gather(allb, bits)
                delta = ref.vote_delta(torch.stack([b.reshape(-1) for b in allb]),
                                       torch.ones(world, dtype=torch.uint8), ref.VOTE_AVERAGE)
                ref.apply_delta_(p, delta, LR, WD)
                ref.momentum_update_(p.grad, m, 0.99)
    oracle_ok = dropout is not None or all(torch.equal(a, b) for a, b in zip(net.parameters(), oracle.parameters()))
    return {"flat": _flat(net), "oracle_ok": oracle_ok, "stats": opt.stats(), "plan_bytes": opt.plan.total_bytes,
            "n_buckets": len(opt.plan.buckets)}


def test_w5_natural_routing_matches_oracle_and_wire_formula():
    from distributed_lion_pytorch_amd.parallel.exchange import wire_bytes_per_step

    world, steps = 5, 3
    res = run_world(_train, world, "a2a", False, steps, None)
    for r in res:
        assert r["oracle_ok"], "parameters differ from the per-tensor average oracle"
        assert torch.equal(r["flat"], res[0]["flat"]), "replicas diverged"
        assert r["stats"]["exchange_impl"] == "AllToAllExchange+counts"
    st = res[0]["stats"]
    assert res[0]["n_buckets"] > 1
    numel, nb = st["numel"], (st["numel"] + 7) // 8
    assert st["wire_bytes_analytic"] == 4 * (1 + 3) * nb // 5  # (W-1)/W * (1+P) planes, P = 3
    # the measured bytes are the same formula over the plan's (padded) plane bytes
    assert st["wire_bytes_recv"] == steps * wire_bytes_per_step(8 * res[0]["plan_bytes"], world, "a2a", vote="average")
    assert st["wire_bytes_recv"] == steps * 4 * (1 + 3) * res[0]["plan_bytes"] // 5
    assert st["wire_bytes_sent"] == st["wire_bytes_recv"]
    assert st["collectives"] == steps * 2 * res[0]["n_buckets"]  # one all-to-all + ONE all-gather per bucket
    assert 0 < numel <= 8 * res[0]["plan_bytes"]


@pytest.mark.parametrize("world", [2, 3])
def test_forced_counts_small_worlds_match_oracle(world):
    res = run_world(_train, world, "a2a", True, 2, None)
    for r in res:
        assert r["oracle_ok"]
        assert torch.equal(r["flat"], res[0]["flat"])
        assert r["stats"]["exchange_impl"] == "AllToAllExchange+counts"
    p = world.bit_length()
    assert res[0]["stats"]["wire_bytes_recv"] == 2 * (world - 1) * (1 + p) * res[0]["plan_bytes"] // world


def test_w3_unforced_keeps_the_allgather_exchange():
    res = run_world(_train, 3, "a2a", False, 1, None)
    for r in res:
        assert r["oracle_ok"]
        assert r["stats"]["exchange_impl"] == "AllGatherExchange"
        assert r["stats"]["wire_bytes_recv"] == 2 * r["plan_bytes"]
        assert r["stats"]["wire_bytes_analytic"] == 2 * ((r["stats"]["numel"] + 7) // 8)


def _dropout_pair(rank, world):
    sched = {1: [0, 1]}
    a = _train(rank, world, "a2a", False, 3, sched)
    b = _train(rank, world, "allgather", False, 3, sched)
    return {"a2a": a["flat"], "allgather": b["flat"], "impl": [a["stats"]["exchange_impl"], b["stats"]["exchange_impl"]]}


def test_w5_simulated_dropout_equals_allgather():
    res = run_world(_dropout_pair, 5)
    for r in res:
        assert r["impl"] == ["AllToAllExchange+counts", "AllGatherExchange"]
        assert torch.equal(r["a2a"], r["allgather"])
        assert torch.equal(r["a2a"], res[0]["a2a"])


def test_wire_bytes_per_step_formula():
    from distributed_lion_pytorch_amd.parallel.exchange import wire_bytes_per_step

    n = 1_000_003
    nb = (n + 7) // 8
    assert wire_bytes_per_step(n, 8, "a2a", vote="average") == 7 * 5 * nb // 8
    assert wire_bytes_per_step(n, 15, "a2a", vote="average") == 14 * 5 * nb // 15
    assert wire_bytes_per_step(n, 4, "a2a", vote="average") == 3 * nb  # W <= 4: the all-gather wire
    assert wire_bytes_per_step(n, 16, "a2a", vote="average") == 15 * nb  # beyond the sliced counter
    assert wire_bytes_per_step(n, 3, "a2a", vote="average", counts=True) == 2 * 3 * nb // 3
    assert wire_bytes_per_step(n, 8, "allgather", vote="average") == 7 * nb
    # the default call is unchanged
    assert wire_bytes_per_step(n, 8, "a2a") == 2 * 7 * nb // 8
    assert wire_bytes_per_step(n, 8, "a2a", vote="majority") == 2 * 7 * nb // 8
    assert wire_bytes_per_step(n, 8, "allgather") == 7 * nb
    assert wire_bytes_per_step(n, 1, "a2a", vote="average") == 0


def _plan(world):
    from distributed_lion_pytorch_amd.optim.executors import TorchExecutor
    from distributed_lion_pytorch_amd.optim.plan import FlatPlan

    plan = FlatPlan([(torch.zeros(5000), 0)], world=world)
    return plan, TorchExecutor(plan)


def test_wide_worlds_keep_the_allgather_fallback():
    from distributed_lion_pytorch_amd.ops import reference as ref
    from distributed_lion_pytorch_amd.parallel.exchange import (AllGatherExchange, AllToAllExchange, make_exchange)

    plan, ex = _plan(16)
    xch = make_exchange("a2a", plan, None, 0, 16, ex, ref.TIE_NEGATIVE, ref.VOTE_AVERAGE)
    assert type(xch) is AllGatherExchange
    assert type(make_exchange("a2a", plan, None, 0, 16, ex, ref.TIE_NEGATIVE, ref.VOTE_AVERAGE,
                              counts=True)) is AllGatherExchange
    with pytest.raises(ValueError):
        AllToAllExchange(plan, None, 0, 16, ex, ref.TIE_NEGATIVE, ref.VOTE_AVERAGE)
    plan15, ex15 = _plan(15)
    x15 = make_exchange("a2a", plan15, None, 0, 15, ex15, ref.TIE_NEGATIVE, ref.VOTE_AVERAGE)
    assert type(x15) is AllToAllExchange and x15.use_counts and x15.n_planes == 4
    assert x15.shard_counts.numel() == 4 * plan15.total_bytes // 15 and x15.counts.numel() == 4 * plan15.total_bytes
    # majority over a2a is untouched by the routing
    xm = make_exchange("a2a", plan15, None, 0, 15, ex15, ref.TIE_ZERO, ref.VOTE_MAJORITY)
    assert type(xm) is AllToAllExchange and not xm.use_counts and xm.need_neg


def test_count_planes_oracle_roundtrip():
    """count_planes -> counted_delta equals vote_delta's average, dead voters masked."""
    from distributed_lion_pytorch_amd.ops import reference as ref

    g = torch.Generator().manual_seed(0)
    for world in (1, 2, 3, 5, 8, 15):
        bits = torch.randint(0, 2, (world, 777), generator=g).bool()
        alive = torch.ones(world, dtype=torch.uint8)
        if world >= 3:
            alive[1] = 0
        cb = ref.count_planes(bits, alive, world)
        assert cb.shape == (world.bit_length(), 777)
        d = ref.counted_delta(cb, int(alive.sum()))
        assert torch.equal(d, ref.vote_delta(bits, alive, ref.VOTE_AVERAGE))
