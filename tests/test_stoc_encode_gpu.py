"""The stochastic sign encoder K3 (``lion_encode_kernel<DT, true>``) against
the integer oracle ``ref.stochastic_bits_exact``, bit for bit: every dtype,
partial lanes and tails, misaligned storage, several buckets, the momentum
store, the fused clip, a coordinate beyond 2^32 and the special values.  The
expectations are computed on the CPU (tests/stoc_cases.py)."""
import itertools
import math

import pytest
import torch

import stoc_cases as sc
from distributed_lion_pytorch_amd.ops import hip
from distributed_lion_pytorch_amd.ops import reference as ref
from distributed_lion_pytorch_amd.optim.executors import HParams, HipExecutor, TorchExecutor
from distributed_lion_pytorch_amd.optim.plan import FlatPlan
from test_kernels_gpu import _assert_close

pytestmark = pytest.mark.gpu

HP = HParams(lr=1e-3, wd=0.1, beta1=sc.BETA1, beta2=sc.BETA2)


@pytest.fixture(autouse=True)
def _need_hip(cuda):
    hip.require()


def _clone(ts):
    return [t.clone() for t in ts]


def _device_case(dtype, cuda, bucket_bytes, sizes=sc.SIZES, seed=0):
    """CPU tensors and plan, their copies on the GPU (same storage offsets)
    and the GPU plan: the two plans have the same layout."""
    ps, gs, ms = sc.tensors(dtype, seed=seed, sizes=sizes)
    cplan = sc.plan_of(ps, bucket_bytes)
    dps, dgs, dms = (sc.to_device(ts, cuda) for ts in (ps, gs, ms))
    plan = sc.plan_of(dps, bucket_bytes)
    assert [(b.byte_off, b.nbytes) for b in plan.buckets] == [(b.byte_off, b.nbytes) for b in cplan.buckets]
    return (ps, gs, ms, cplan), (dps, dgs, dms, plan)


def _encode_all(plan, gs, ms, rr, update_m=True, stochastic=True, gscale=None, seed=sc.SEED, step=sc.STEP):
    """The kernel's send buffer for the whole plan: prefilled with 0xAB, the
    buckets' padding (which no encoder writes) cleared first."""
    bits = torch.full((plan.total_bytes,), 0xAB, dtype=torch.uint8, device=plan.device)
    hx = HipExecutor(plan)
    meta = plan.meta(gs, ms)
    for b in plan.buckets:
        bits[b.byte_off + sc.used_bytes(b):b.byte_off + b.nbytes] = 0
        hx.encode(meta, b, bits[b.byte_off:b.byte_off + b.nbytes], HP, update_m=update_m, stochastic=stochastic,
                  rr=rr, seed=seed, step=step, gscale=gscale)
    torch.cuda.synchronize()
    return bits


def _assert_planes_equal(plan, got, want):
    got = got.cpu()
    for b in plan.buckets:
        sl = slice(b.byte_off, b.byte_off + b.nbytes)
        bad = (got[sl] != want[sl]).nonzero().flatten()
        assert torch.equal(got[sl], want[sl]), (b.index, bad.numel(), bad[:8].tolist())


# ------------------------------------------------------------------ Test A
@pytest.mark.parametrize("bucket_bytes", sc.BUCKET_BYTES)
@pytest.mark.parametrize("rr", sc.RRS)
@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_bits_match_the_oracle(dtype, rr, bucket_bytes, cuda):
    """Every byte of the send buffer equals the packed oracle bits: no
    coordinate is excluded, and the padding bits of each tensor's 2048-bit
    region come back 0 from the 0xAB prefill.  The data puts 3.4 - 4.5 % of the
    coordinates on each clamp and 91 - 93 % in the open interval (sc.shares,
    from the oracle)."""
    (ps, gs, ms, cplan), (dps, dgs, dms, plan) = _device_case(dtype, cuda, bucket_bytes)
    assert len(plan.buckets) == (1 if bucket_bytes == 1 << 13 else 4)
    low, mid, high = sc.shares(gs, ms, rr)
    print(f"{dtype} rr={rr:.4f}: low clamp {low:.4f}, open interval {mid:.4f}, high clamp {high:.4f}")
    assert low >= 0.01 and high >= 0.01 and mid >= 0.5
    want = sc.oracle_planes(cplan, gs, ms, rr)
    got = _encode_all(plan, dgs, dms, rr)
    _assert_planes_equal(plan, got, want)


def test_aten_hip_interp_is_the_kernels_expression(cuda):
    """bf16: ``interp`` through ATen-HIP equals ``interp_exact`` computed on
    the CPU bit for bit (ATen's CPU add_ rounds alpha to bf16 and does not)."""
    _, gs, ms = sc.tensors(torch.bfloat16)
    g, m = torch.cat(gs), torch.cat(ms)
    assert torch.equal(ref.interp(g.to(cuda), m.to(cuda), sc.BETA1).cpu(), ref.interp_exact(g, m, sc.BETA1))


# ------------------------------------------------------------------ Test B
@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_momentum_under_stoc(dtype, cuda):
    """update_m=True stores the momentum of the deterministic encode, bit for
    bit, which is ATen's within the usual bounds; update_m=False leaves it."""
    rr = sc.RRS[1]
    _, (dps, dgs, dms, plan) = _device_case(dtype, cuda, 1 << 11)
    m0 = _clone(dms)
    _encode_all(plan, dgs, dms, rr, update_m=False)
    for a, b in zip(dms, m0):
        assert sc.same_bits(a, b).all()
    _encode_all(plan, dgs, dms, rr, update_m=True)
    m_stoc = _clone(dms)
    for t, s in zip(dms, m0):
        t.copy_(s)
    _encode_all(plan, dgs, dms, 0.0, update_m=True, stochastic=False)
    for a, b, g, m in zip(m_stoc, dms, dgs, m0):
        assert sc.same_bits(a, b).all()
        ref.momentum_update_(g, m, sc.BETA2)
        _assert_close(a, m, dtype)


# ------------------------------------------------------------------ Test C
@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_gscale_under_stoc(dtype, cuda):
    """The fused clip: bits and momentum are those of gradients scaled in
    place first, round(g * coef) in the tensors' dtype."""
    rr = sc.RRS[1]
    (ps, gs, ms, cplan), (dps, dgs, dms, plan) = _device_case(dtype, cuda, 1 << 11, seed=2)
    coef = torch.tensor(0.37, dtype=torch.float32)
    gscale = torch.stack([torch.tensor(123.0), coef]).to(cuda)  # [norm, coefficient]
    scaled = [(g.float() * coef).to(dtype) for g in gs]
    assert any(not torch.equal(a, b) for a, b in zip(scaled, gs))
    want = sc.oracle_planes(cplan, scaled, ms, rr)
    m0 = _clone(dms)
    got = _encode_all(plan, dgs, dms, rr, gscale=gscale)
    _assert_planes_equal(plan, got, want)
    m_fused = _clone(dms)
    for t, s in zip(dms, m0):
        t.copy_(s)
    got2 = _encode_all(plan, sc.to_device(scaled, cuda), dms, rr)
    assert torch.equal(got, got2)
    for a, b in zip(m_fused, dms):
        assert sc.same_bits(a, b).all()


# ------------------------------------------------------------------ Test D
def test_high_counter_word(cuda):
    """A coordinate base beyond 2^32 reaches Philox counter word 1."""
    rr, cbase, dtype = sc.RRS[1], 2 ** 33 + 8 * 4096, torch.bfloat16
    (ps, gs, ms, cplan), (dps, dgs, dms, plan) = _device_case(dtype, cuda, 1 << 13, sizes=[2049])
    b = plan.buckets[0]
    bits = torch.full((plan.total_bytes,), 0xAB, dtype=torch.uint8, device=cuda)
    bits[sc.used_bytes(b):] = 0
    hip.ops().lion_encode(plan.meta(dgs, dms), plan.seg_off, plan.chunk_off + 2 * b.chunk_off, b.n_chunks,
                          hip.DTYPE_CODE[dtype], bits, sc.BETA1, 1.0 - sc.BETA1, sc.BETA2, 1.0 - sc.BETA2, False, True,
                          rr, sc.SEED, sc.STEP, None, cbase)
    torch.cuda.synchronize()
    want = sc.oracle_planes(cplan, gs, ms, rr, cbase=cbase)
    _assert_planes_equal(plan, bits, want)
    assert not torch.equal(want, sc.oracle_planes(cplan, gs, ms, rr, cbase=8 * 4096))


# ------------------------------------------------------------------ Test E
def _special_case(cuda):
    p, g, m = sc.special_lattice()
    plan = FlatPlan([(p, 0)], world=1, bucket_bytes=1 << 13)
    dp, dg, dm = p.to(cuda), g.to(cuda), m.to(cuda)
    dplan = FlatPlan([(dp, 0)], world=1, bucket_bytes=1 << 13, device=cuda)
    return (p, g, m, plan), (dp, dg, dm, dplan)


def _all_same(a, b, what, g, m):
    ok = sc.same_bits(a.cpu(), b.cpu())
    bad = (~ok).nonzero().flatten()[:6]
    assert ok.all(), (what, int((~ok).sum()), [(g[i].item(), m[i].item(), a[i].item(), b[i].item()) for i in bad])


def test_special_values_k3(cuda):
    """One full chunk and a tail of every (g, m) pair of +-0, +-subnormal,
    +-smallest normal, +-1, +-largest finite, +-inf and NaN: K3's bits are the
    oracle's (NaN -> 0, +inf -> 1, -inf -> 0, u = 0 -> the coin)."""
    (p, g, m, cplan), (dp, dg, dm, plan) = _special_case(cuda)
    for rr in sc.RRS:
        want = sc.oracle_planes(cplan, [g], [m], rr)
        got = _encode_all(plan, [dg], [dm], rr, update_m=False)
        _assert_planes_equal(plan, got, want)
    u = ref.interp_exact(g, m, sc.BETA1).float()
    assert torch.isnan(u).any() and (u == math.inf).any() and (u == -math.inf).any() and (u == 0).any()


def test_special_values_k1_k0(cuda):
    """The same lattice through the deterministic kernels: K1's bits and
    momentum against the torch executor, K0's p and m against ref.update_fn
    (both ATen on the device), bit patterns with NaN matching any NaN."""
    (p, g, m, cplan), (dp, dg, dm, plan) = _special_case(cuda)
    m0 = dm.clone()
    b = plan.buckets[0]
    # K1
    got = _encode_all(plan, [dg], [dm], 0.0, stochastic=False)
    m_ref = m0.clone()
    want = torch.zeros_like(got)
    TorchExecutor(plan).encode(None, b, want, HP, grads=[dg], moms=[m_ref])
    assert torch.equal(got, want), (got != want).nonzero().flatten()[:8].tolist()
    _all_same(dm, m_ref, "K1 momentum", g, m)
    # K0
    dm.copy_(m0)
    p_ref, m_ref = dp.clone(), m0.clone()
    HipExecutor(plan).local(plan.meta([dg], [dm]), b, HP)
    ref.update_fn(p_ref, dg, m_ref, HP.lr, HP.wd, HP.beta1, HP.beta2)
    torch.cuda.synchronize()
    _all_same(dm, m_ref, "K0 momentum", g, m)
    _all_same(dp, p_ref, "K0 parameter", g, m)


# --------------------------------------------------------------- thresholds
@pytest.mark.parametrize("rr", sc.RRS)
def test_every_draw_at_its_threshold(rr, cuda):
    """fp32, beta1 = 1 (u = m): each m is one fp32 step to either side of the
    value at which its own draw flips the bit (sc.threshold_case), so the
    planes are 0x55 bytes only if the kernel's probability, draw and compare
    are the oracle's to the last bit."""
    n = 8200
    g, m, want = sc.threshold_case(rr, n=n)
    hp = HParams(lr=1e-3, wd=0.0, beta1=1.0, beta2=sc.BETA2)
    dg, dm = g.to(cuda), m.to(cuda)
    plan = FlatPlan([(dg, 0)], world=1, bucket_bytes=1 << 13, device=cuda)
    bits = torch.full((plan.total_bytes,), 0xAB, dtype=torch.uint8, device=cuda)
    HipExecutor(plan).encode(plan.meta([dg], [dm]), plan.buckets[0], bits, hp, update_m=False, stochastic=True, rr=rr,
                             seed=sc.SEED, step=sc.STEP)
    torch.cuda.synchronize()
    got = ref.unpack_bits(bits.cpu())
    assert torch.equal(got[:n], want), int((got[:n] != want).sum())
    assert want[0::2].all() and not want[1::2].any() and not got[n:].any()


# ------------------------------------------------------------------ Test F
@pytest.mark.parametrize("bucket_bytes", sc.BUCKET_BYTES)
@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_backends_agree(dtype, bucket_bytes, cuda):
    """The HIP executor on the GPU and the torch executor on the CPU write the
    same planes for every bucket of the plan."""
    rr = sc.RRS[1]
    (ps, gs, ms, cplan), (dps, dgs, dms, plan) = _device_case(dtype, cuda, bucket_bytes, seed=4)
    got = _encode_all(plan, dgs, dms, rr)
    want = torch.zeros(cplan.total_bytes, dtype=torch.uint8)
    tx = TorchExecutor(cplan)
    for b in cplan.buckets:
        tx.encode(None, b, want[b.byte_off:b.byte_off + b.nbytes], HP, stochastic=True, rr=rr, seed=sc.SEED,
                  step=sc.STEP, grads=gs, moms=_clone(ms))
    _assert_planes_equal(plan, got, want)


def test_identical_buckets_differ(cuda):
    """Four buckets of one 8192-element tensor each, g = m = 0 (p = 1/2): each
    pair of planes agrees on a share a of its n = 8192 bits with |a - 1/2| <
    6 * 0.5 / sqrt(n).  A bucket-relative counter makes it 1.0."""
    n = 8192
    ps = [torch.zeros(n, dtype=torch.bfloat16, device=cuda) for _ in range(4)]
    plan = FlatPlan([(p, 0) for p in ps], world=sc.WORLD, bucket_bytes=n // 8, device=cuda)
    assert len(plan.buckets) == 4 and all(b.numel == n for b in plan.buckets)
    bits = _encode_all(plan, [torch.zeros_like(p) for p in ps], _clone(ps), 2.0)
    planes = ref.unpack_bits(bits.cpu().view(4, n // 8))
    for i, j in itertools.combinations(range(4), 2):
        a = (planes[i] == planes[j]).double().mean().item()
        print(f"buckets {i}, {j}: agree on {a:.4f}")
        assert abs(a - 0.5) < 6 * 0.5 / math.sqrt(n), (i, j, a)
