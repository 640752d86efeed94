"""Average voting over the all-to-all exchange on one GPU: the shard count
kernel (K4c, ``vote_count``) against the oracle, and the counted apply (K2
mode 3) bit for bit against the byte-spread average kernel (mode 1) fed the
same W fake voter planes -- several buckets, shards that are no multiple of a
chunk's 1024 bytes (a chunk straddles two shards), a dead voter, a tensor
that is not 16-byte aligned, with and without the agreement telemetry."""
import copy

import pytest
import torch

from distributed_lion_pytorch_amd.ops import hip
from distributed_lion_pytorch_amd.ops import reference as ref
from distributed_lion_pytorch_amd.optim.executors import HParams, HipExecutor, TorchExecutor
from distributed_lion_pytorch_amd.optim.plan import FlatPlan

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 2048, 2049, 8192, 8193, 3 * 8192 + 5, 40000]
WORLDS = [1, 2, 3, 5, 8, 15]
DTYPES = [torch.bfloat16, torch.float32, torch.float16]
BUCKET_BYTES = 1 << 13
HP = HParams(lr=3e-3, wd=0.05, beta1=0.9, beta2=0.99)


@pytest.fixture(autouse=True)
def _need_hip(cuda):
    hip.require()


def _params(dtype, dev):
    g = torch.Generator(device="cpu").manual_seed(5)
    ps = []
    for i, n in enumerate(SIZES):
        ps.append(torch.randn(n, generator=g).to(dtype).to(dev))
    return _misalign(ps)


def _misalign(ps):
    """The second tensor becomes a view one element into its (device) storage: not 16-byte aligned."""
    ps[1] = torch.cat([ps[1].new_zeros(1), ps[1]])[1:]
    assert ps[1].data_ptr() % 16 != 0 and ps[1].is_contiguous()
    return ps


def _plan(ps, world, dev):
    return FlatPlan([(p, 0) for p in ps], world=world, bucket_bytes=BUCKET_BYTES, device=dev)


def _alive(world, dev):
    alive = torch.ones(world, dtype=torch.uint8, device=dev)
    if world >= 3:
        alive[1] = 0
    return alive


def _rebind(bucket, new_params):
    b2 = copy.copy(bucket)
    b2.segments = [copy.copy(s) for s in bucket.segments]
    for s in b2.segments:
        s.param = new_params[s.index]
    return b2


def _assert_close(a, b, dtype, exact=True):
    """The tolerances of test_kernels_gpu.py (its ``exact=False`` branch is the
    one for the fractional average deltas against the ATen oracle)."""
    if dtype == torch.float32:
        torch.testing.assert_close(a, b, rtol=2e-7, atol=1e-7)
    elif dtype == torch.float16:
        torch.testing.assert_close(a.float(), b.float(), rtol=1e-3, atol=1e-5)
    elif not exact:
        torch.testing.assert_close(a.float(), b.float(), rtol=8e-3, atol=1e-5)
        assert (a != b).float().mean().item() < 1e-3
    else:
        assert torch.equal(a, b), (a - b).abs().max()


_CACHE = {}


def _voters(world, dev):
    """Per world, computed once and left unchanged: the W fake voter planes
    (seeded CPU generator), per bucket the all-gather layout [W][nbytes], the
    HIP count planes [W][P][shard] and K4c's tie count."""
    if world in _CACHE:
        return _CACHE[world]
    plan = _plan([torch.empty(n) for n in SIZES], world, torch.device("cpu"))
    assert len(plan.buckets) > 1
    # a chunk (1024 plane bytes) straddles two shards somewhere
    assert any((b.nbytes // world) % 1024 != 0 for b in plan.buckets)
    gen = torch.Generator(device="cpu").manual_seed(100 + world)
    planes = torch.randint(0, 256, (world, plan.total_bytes), generator=gen, dtype=torch.uint8).to(dev)
    alive = _alive(world, dev)
    npl = world.bit_length()
    hx = HipExecutor(plan)
    ties = torch.zeros(1, dtype=torch.int64, device=dev)
    gathered, counts, guard_ok = [], [], True
    for b in plan.buckets:
        pl = planes[:, b.byte_off:b.byte_off + b.nbytes].contiguous()  # [W][nbytes]
        shard = b.nbytes // world
        blocks = []
        for r in range(world):  # what rank r holds after the all-to-all: its shard of every plane
            recv = pl[:, r * shard:(r + 1) * shard].contiguous().reshape(-1)
            out = torch.full((npl * shard + 64,), 0xAB, dtype=torch.uint8, device=dev)
            hx.vote_count(recv, shard, alive, out, ties)
            guard_ok = guard_ok and bool((out[npl * shard:] == 0xAB).all())
            blocks.append(out[:npl * shard])
        gathered.append(pl.reshape(-1))
        counts.append(torch.cat(blocks))  # [W][P][shard]
    torch.cuda.synchronize()
    _CACHE[world] = {"planes": planes, "alive": alive, "gathered": gathered, "counts": counts,
                     "ties": int(ties.item()), "guard_ok": guard_ok, "bucket_bytes": [b.nbytes for b in plan.buckets]}
    return _CACHE[world]


@pytest.mark.parametrize("world", WORLDS)
def test_vote_count_matches_oracle(world, cuda):
    v = _voters(world, cuda)
    assert v["guard_ok"], "vote_count wrote past its P planes"
    npl = world.bit_length()
    n_live = int(v["alive"].sum())
    ties = 0
    for pl, cnt, nbytes in zip(v["gathered"], v["counts"], v["bucket_bytes"]):
        shard = nbytes // world
        bits = ref.unpack_bits(pl.view(world, nbytes))  # bool[W, nbytes * 8]
        got = ref.unpack_bits(cnt.view(world, npl, shard))  # bool[W(shard), P, shard * 8]
        for r in range(world):
            want = ref.count_planes(bits[:, r * shard * 8:(r + 1) * shard * 8], v["alive"], world)
            assert want.shape == (npl, shard * 8)
            assert torch.equal(got[r], want), f"shard {r}"
        twice = 2 * bits[v["alive"].bool()].to(torch.int64).sum(0)
        ties += int(((twice == n_live) & (n_live > 0)).sum())
    assert v["ties"] == ties
    assert (v["ties"] > 0) == (n_live % 2 == 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32", "fp16"])
@pytest.mark.parametrize("world", WORLDS)
def test_counted_apply_equals_byte_kernel(world, dtype, cuda):
    v = _voters(world, cuda)
    alive = v["alive"]
    base = _params(dtype, cuda)
    plan = _plan(base, world, cuda)
    assert [b.nbytes for b in plan.buckets] == v["bucket_bytes"]

    def run(executor_cls, mode, telemetry):
        ps = _misalign([p.clone() for p in base])
        pl2 = _plan(ps, world, cuda)
        ex = executor_cls(pl2)
        meta = pl2.meta(ps, ps) if executor_cls is HipExecutor else None
        agree = torch.zeros(2, dtype=torch.int64, device=cuda) if telemetry else None
        for b, gathered, cnt in zip(pl2.buckets, v["gathered"], v["counts"]):
            own = gathered[:b.nbytes] if telemetry else None
            if mode == ref.VOTE_COUNTED:
                ex.apply(meta, b, cnt, b.nbytes // world, alive, mode, 0, None, HP, own=own, agree=agree)
            else:
                ex.apply(meta, b, gathered, b.nbytes, alive, mode, 0, None, HP, own=own, agree=agree)
        torch.cuda.synchronize()
        return ps, (agree.tolist() if telemetry else None)

    want, agree_want = run(HipExecutor, ref.VOTE_AVERAGE, True)  # the byte kernel: the independent reference
    assert any(not torch.equal(a, b) for a, b in zip(want, base))
    pair, _ = run(HipExecutor, ref.VOTE_COUNTED, False)  # two-chunks-per-block kernel
    for a, b in zip(pair, want):
        assert torch.equal(a, b), (a.float() - b.float()).abs().max()
    one, agree_got = run(HipExecutor, ref.VOTE_COUNTED, True)  # one-chunk kernel with telemetry
    for a, b in zip(one, want):
        assert torch.equal(a, b), (a.float() - b.float()).abs().max()
    assert agree_got[0] == agree_want[0]
    assert agree_got[1] == 0  # the ties were counted by K4c on the shard
    oracle, agree_t = run(TorchExecutor, ref.VOTE_COUNTED, True)
    for a, b in zip(pair, oracle):
        _assert_close(a, b, dtype, exact=False)
    assert agree_t == agree_got
