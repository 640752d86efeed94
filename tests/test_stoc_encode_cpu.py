"""The stochastic sign encoder's integer oracle (CPU): Philox known answers,
the lane layout of the draws, the exact interpolation, the probability law,
special values, independent draws per bucket on the torch backend, and a
reproducible end-to-end run."""
import itertools
import math
from fractions import Fraction

import pytest
import torch
import torch.distributed as dist

import stoc_cases as sc
from distributed_lion_pytorch_amd import Lion
from distributed_lion_pytorch_amd.ops import reference as ref
from distributed_lion_pytorch_amd.optim.executors import HParams, TorchExecutor, coord_base
from distributed_lion_pytorch_amd.optim.plan import FlatPlan

M32 = 0xFFFFFFFF


# ------------------------------------------------------------- 1. Philox
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_known_answers():
    """The three published Philox4x32-10 vectors, on Python ints and on int64
    tensors (all three counters in one call)."""
    for ctr, key, out in KAT:
        assert ref.philox4x32_10(ctr, key) == out
    ctr = [torch.tensor([k[0][i] for k in KAT], dtype=torch.int64) for i in range(4)]
    key = [torch.tensor([k[1][i] for k in KAT], dtype=torch.int64) for i in range(2)]
    got = ref.philox4x32_10(ctr, key)
    for i in range(4):
        assert got[i].dtype == torch.int64 and got[i].tolist() == [k[2][i] for k in KAT]


# ----------------------------------------------------------- 2. stoc_unit
def _unit(word: int) -> float:
    return (word >> 8) * 2.0 ** -24


def test_stoc_unit_lane_layout():
    seed, step = (0x89ABCDEF << 32) | 0x01234567, 5
    key = (seed & M32, seed >> 32)
    u = ref.stoc_unit(torch.arange(16, dtype=torch.int64), seed, step)
    assert u.dtype == torch.float32 and 0 <= u.min().item() and u.max().item() < 1
    want = []
    for c8 in (0, 8):  # two counters per 8 coordinates, the words in the order x, y, z, w
        for call in (0, 1):
            want += [_unit(w) for w in ref.philox4x32_10((c8, 0, step, call), key)]
    assert u.tolist() == want
    # a coordinate >= 2^32 changes counter word 1
    base = (3 << 32) + 4096
    hi = ref.stoc_unit(base + torch.arange(8, dtype=torch.int64), seed, step)
    assert hi.tolist() == [_unit(w) for call in (0, 1) for w in ref.philox4x32_10((4096, 3, step, call), key)]
    lo = ref.stoc_unit(4096 + torch.arange(8, dtype=torch.int64), seed, step)
    assert (hi != lo).all()
    # step and each half of the seed change the draw; the step enters as 32 bits
    c = torch.arange(4096, dtype=torch.int64)
    u = ref.stoc_unit(c, seed, step)
    for other in (ref.stoc_unit(c, seed, step + 1), ref.stoc_unit(c, seed ^ 1, step),
                  ref.stoc_unit(c, seed ^ (1 << 32), step)):
        assert (other != u).double().mean().item() > 0.99
    assert torch.equal(ref.stoc_unit(c, seed, step + (1 << 32)), u)
    assert torch.equal(ref.stoc_unit(c.view(64, 64), seed, step), u)  # any shape in, flat out


# -------------------------------------------------------- 3. interp_exact
def test_interp_exact_is_the_correctly_rounded_expression():
    """rnd(fma32(g, fp32(1 - b1), rnd(fp32(m) * fp32(b1)))) against rational
    arithmetic, at the optimizer's beta1 = 0.9, in every dtype; for fp32 that
    is ``_fma32`` of the same operands."""
    b1 = 0.9
    b1f = Fraction(torch.tensor(b1, dtype=torch.float32).item())
    omb1f = Fraction(torch.tensor(1 - b1, dtype=torch.float32).item())
    for dtype in sc.DTYPES:
        _, gs, ms = sc.tensors(dtype, sizes=[300])
        g, m = gs[0], ms[0]
        got = ref.interp_exact(g, m, b1)
        assert got.dtype == dtype and got.shape == g.shape
        if dtype == torch.float32:
            assert torch.equal(got, ref._fma32(1 - b1, g, m * torch.tensor(b1, dtype=torch.float32)))
        for i in range(300):
            mb = Fraction(_nearest(Fraction(m[i].item()) * b1f, torch.float32, dtype).item())
            want = _nearest(Fraction(g[i].item()) * omb1f + mb, torch.float32, dtype)
            assert got[i].item() == want.item(), (dtype, i)


def _nearest(x: Fraction, *dtypes) -> torch.Tensor:
    """x rounded to nearest-even in dtypes[0], that value then in dtypes[1]:
    the fp64 quotient of the fraction, pushed off the midpoints it may have
    rounded onto (round to odd), cannot double-round into a 24-bit format."""
    q = torch.tensor(x.numerator / x.denominator, dtype=torch.float64)
    exact = Fraction(q.item())
    if exact != x:
        b = q.view(torch.int64)
        if (exact > x) == (x > 0):  # |q| > |x|: one ulp toward zero first
            b = b - 1
        q = (b | 1).view(torch.float64)
    for dt in dtypes:
        q = q.to(dt)
    return q


def test_interp_exact_equals_aten_interp_for_bf16():
    """``interp`` (ATen) and the kernels' expression agree bit for bit on bf16
    where ATen evaluates the same fp32 expression.  On the CPU ATen rounds
    add_'s alpha to bf16 first (0.1 -> 0.10009765625), so the equality is
    asserted at beta1 = 0.875: both factors are bf16 numbers and the products
    by 0.125 are exact, an fma or a multiply and an add.  At beta1 = 0.9 the
    CPU's ``interp`` follows the bf16 alpha (asserted too, so that a change of
    ATen shows up here); the GPU test asserts the equality with ATen-HIP's
    ``interp`` at 0.9, where alpha stays fp32."""
    _, gs, ms = sc.tensors(torch.bfloat16)
    g, m = torch.cat(gs), torch.cat(ms)
    assert torch.equal(ref.interp_exact(g, m, 0.875), ref.interp(g, m, 0.875))
    alpha = torch.tensor(1 - 0.9, dtype=torch.bfloat16).float()
    mb = (m.float() * torch.tensor(0.9, dtype=torch.float32)).bfloat16().float()
    cpu_expr = (mb + alpha * g.float()).bfloat16()
    assert (cpu_expr != ref.interp(g, m, 0.9)).double().mean().item() < 1e-3


# ------------------------------------------------------ 4. probability law
def test_probability_law():
    """Constant u at -rr .. 2rr with rr = 2 (0.5 / rr exact): the bit mean is
    within 6 sigma of p = clamp((u + rr) / 2rr) over n = 2^16 coordinates, and
    exactly 0 or 1 at the clamped ends."""
    rr, n = 2.0, 1 << 16
    c = torch.arange(n, dtype=torch.int64)
    zero = torch.zeros(n)
    for u in (-rr, -rr / 2, 0.0, rr / 2, rr, 2 * rr):
        # beta1 = 0.5: interp_exact(2u, 0) = u exactly
        bits = ref.stochastic_bits_exact(torch.full((n,), 2 * u), zero, 0.5, rr, c, seed=9, step=1)
        p = min(1.0, max(0.0, (u + rr) / (2 * rr)))
        mean = bits.double().mean().item()
        print(f"u = {u:+.1f}: mean bit {mean:.5f}, p = {p}")
        if p in (0.0, 1.0):
            assert mean == p
        else:
            assert abs(mean - p) < 6 * math.sqrt(p * (1 - p) / n)


def test_special_values():
    n = 4096
    c = torch.arange(n, dtype=torch.int64)
    half = ref.stoc_unit(c, 4, 2) < 0.5
    assert abs(half.double().mean().item() - 0.5) < 6 * 0.5 / math.sqrt(n)
    zero = torch.zeros(n)
    for u, want in ((float("nan"), torch.zeros(n, dtype=torch.bool)), (float("inf"), torch.ones(n, dtype=torch.bool)),
                    (float("-inf"), torch.zeros(n, dtype=torch.bool)), (0.0, half), (-0.0, half)):
        for dtype in sc.DTYPES:
            g = torch.full((n,), u, dtype=dtype)
            bits = ref.stochastic_bits_exact(g, zero.to(dtype), 0.9, 2.0, c, seed=4, step=2)
            assert bits.dtype == torch.bool and torch.equal(bits, want), (u, dtype)


@pytest.mark.parametrize("rr", sc.RRS)
def test_threshold_case_sits_on_the_edge_of_every_draw(rr):
    """The data of the GPU threshold test: bits alternate 1, 0, one fp32 step
    of m apart, and near-misses of the probability do flip them -- the
    division by 2 rr where 0.5 / rr is inexact, ``<=`` for ``<``, and a draw
    of 23 bits."""
    n = 2048
    g, m, want = sc.threshold_case(rr, n=n)
    c = torch.arange(n, dtype=torch.int64)
    assert torch.equal(ref.stochastic_bits_exact(g, m, 1.0, rr, c, sc.SEED, sc.STEP), want)
    assert want[0::2].all() and not want[1::2].any()
    assert torch.equal(ref.interp_exact(g, m, 1.0), m)
    unit = ref.stoc_unit(c, sc.SEED, sc.STEP)
    rr32 = torch.tensor(rr, dtype=torch.float32)
    pr = ((m + rr32) * (torch.tensor(0.5) / rr32)).clamp(0, 1)
    flips = {"<=": ((unit <= pr) != want).sum().item(),
             "/ (2 rr)": ((unit < ((m + rr32) / (2 * rr32)).clamp(0, 1)) != want).sum().item(),
             "23 bits": (((unit * 2 ** 23).floor() * 2.0 ** -23 < pr) != want).sum().item()}
    print(rr, flips)
    assert flips["<="] > n // 8 and flips["23 bits"] > n // 8
    if rr != 2.0:  # at rr = 2 both forms are exact
        assert flips["/ (2 rr)"] > 0


# ------------------------------------------- 5. independent draws per bucket
def _four_bucket_planes(seed, step, rr=2.0):
    ps = [torch.zeros(4096, dtype=torch.bfloat16) for _ in range(4)]
    plan = FlatPlan([(p, 0) for p in ps], world=1, bucket_bytes=512)
    assert [b.byte_off for b in plan.buckets] == [0, 512, 1024, 1536]
    gs, ms = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    tx = TorchExecutor(plan)
    bits = torch.zeros(plan.total_bytes, dtype=torch.uint8)
    hp = HParams(lr=1e-3, wd=0.0, beta1=0.9, beta2=0.99)
    for b in plan.buckets:
        tx.encode(None, b, bits[b.byte_off:b.byte_off + b.nbytes], hp, stochastic=True, rr=rr, seed=seed, step=step,
                  grads=gs, moms=ms)
    return ref.unpack_bits(bits.view(4, 512))  # bool[4, 4096]


def _rank_seed(seed, rank):  # Lion._encode_launch
    return (seed * 0x9E3779B1 + rank * 0x632BE59BD9B4E019 + 1) & 0x7FFFFFFFFFFFFFFF


def test_buckets_draw_independently_on_the_torch_backend():
    """Four buckets of identical layout and data (g = m = 0: p = 1/2): every
    pair agrees on about half of its 4096 bits.  With a bucket-relative
    counter (or a generator re-seeded per bucket) the share is 1.0."""
    planes = _four_bucket_planes(_rank_seed(7, 0), 0)
    bound = 6 * 0.5 / math.sqrt(4096)
    assert abs(planes.double().mean().item() - 0.5) < 6 * 0.5 / math.sqrt(4 * 4096)
    for i, j in itertools.combinations(range(4), 2):
        a = (planes[i] == planes[j]).double().mean().item()
        print(f"buckets {i}, {j}: agree on {a:.4f}")
        assert abs(a - 0.5) < bound, (i, j, a)
    # the rank term of the seed and the step both give other planes, the same arguments the same ones
    assert torch.equal(planes, _four_bucket_planes(_rank_seed(7, 0), 0))
    for other in (_four_bucket_planes(_rank_seed(7, 1), 0), _four_bucket_planes(_rank_seed(7, 0), 1)):
        assert abs((planes == other).double().mean().item() - 0.5) < 6 * 0.5 / math.sqrt(4 * 4096)


# ------------------------------------------------------------ 6. end to end
def _run_lion(seed=3, steps=3):
    """One rank that votes with itself: the encode -> exchange -> apply path
    of the torch backend, checked step by step against the oracle at the
    plan's global coordinates."""
    lr, wd, b1, b2, mgn = 1e-2, 0.1, 0.9, 0.99, 1.0
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(n).to(torch.bfloat16)) for n in (2100, 33, 2048)]
    shadow = [p.detach().clone() for p in params]
    moms = [torch.zeros_like(p) for p in shadow]
    opt = Lion(params, lr=lr, weight_decay=wd, betas=(b1, b2), backend="torch", max_grad_norm=mgn,
               bucket_mb=0.0005, seed=seed)
    opt._force_vote = True
    gen = torch.Generator().manual_seed(1)
    for step in range(steps):
        for p in params:
            p.grad = torch.randn(p.shape, generator=gen).to(torch.bfloat16)
        opt.step()
        for b in opt.plan.buckets:
            for s in b.segments:
                p, g, m = shadow[s.index], params[s.index].grad, moms[s.index]
                coords = coord_base(b) + s.bit_off + torch.arange(s.numel, dtype=torch.int64)
                bits = ref.stochastic_bits_exact(g, m, b1, (1 + 1 / b1) * mgn, coords, _rank_seed(seed, 0), step)
                ref.apply_delta_(p, bits.float() * 2 - 1, lr, wd)
                ref.momentum_update_(g, m, b2)
    assert len(opt.plan.buckets) > 1
    for p, q in zip(params, shadow):
        assert torch.equal(p.detach(), q)
    return [p.detach().clone() for p in params]


def test_end_to_end_is_reproducible(tmp_path):
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/rdzv", rank=0, world_size=1)
    try:
        a, b, c = _run_lion(), _run_lion(), _run_lion(seed=4)
    finally:
        dist.destroy_process_group()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert any(not torch.equal(x, y) for x, y in zip(a, c))
