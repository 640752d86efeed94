"""Shared data of the stochastic-encode (K3) tests: the tensors, the plans and
the oracle's bit planes, all built on the CPU so that the GPU test compares the
kernel with something the kernel had no part in."""
import torch

from distributed_lion_pytorch_amd.ops import reference as ref
from distributed_lion_pytorch_amd.optim.executors import _region_bytes, coord_base
from distributed_lion_pytorch_amd.optim.plan import FlatPlan

# one element, a partial lane, one lane, lanes + tail, around one 2048-bit region, one full chunk (the fast path
# of the deterministic kernel), a chunk + 1, several chunks with a tail
SIZES = [1, 7, 8, 13, 2047, 2048, 2049, 8192, 8193, 20000]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
WORLD = 4
# 1 << 13 holds all of SIZES in one bucket (55296 bits); 1 << 11 cuts them into four buckets with non-zero byte
# offsets and padded ends, which is what tells a global coordinate from a bucket-relative one
BUCKET_BYTES = [1 << 13, 1 << 11]
BETA1, BETA2 = 0.9, 0.99
RRS = [2.0, (1 + 1 / 0.9) * 1.0]  # 0.5 / rr exact, and Lion(max_grad_norm=1.0)'s value
SEED = 0x1234_5678_9ABC_DEF1 & 0x7FFFFFFFFFFFFFFF  # both key words non-zero
STEP = 3


def misaligned(i: int) -> bool:
    """Every third tensor is stored one element off a 16-byte boundary."""
    return i % 3 == 1


def offset_by_one(t: torch.Tensor) -> torch.Tensor:
    """The same values in storage that starts one element before them."""
    buf = t.new_zeros(t.numel() + 1)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


def tensors(dtype, seed=0, sizes=SIZES):
    """(p, g, m) lists on the CPU.  u = 0.9 m + 0.1 g has a standard deviation
    of about 1.15, i.e. 0.58 rr at rr = 2 and 0.55 rr at rr = 2.11: u / rr
    spans about [-2.4, 2.4], each clamp takes 3 - 4 % of the coordinates and
    the open interval 92 - 93 % (``shares`` measures it)."""
    gen = torch.Generator().manual_seed(seed)
    ps, gs, ms = [], [], []
    for i, n in enumerate(sizes):
        trio = [torch.randn(n, generator=gen).to(dtype), (torch.randn(n, generator=gen) * 4.0).to(dtype),
                (torch.randn(n, generator=gen) * 1.2).to(dtype)]
        if misaligned(i):
            trio = [offset_by_one(t) for t in trio]
        ps.append(trio[0])
        gs.append(trio[1])
        ms.append(trio[2])
    return ps, gs, ms


def to_device(ts, dev):
    """Copies on ``dev`` that keep a one-element storage offset (a plain
    ``.to(dev)`` of a view lands in fresh, aligned storage)."""
    out = []
    for t in ts:
        d = t.to(dev)
        if t.storage_offset():
            d = offset_by_one(d)
            assert d.data_ptr() % 16 != 0
        out.append(d)
    return out


def plan_of(ps, bucket_bytes, world=WORLD):
    return FlatPlan([(p, 0) for p in ps], world=world, bucket_bytes=bucket_bytes, device=ps[0].device)


def used_bytes(b) -> int:
    """Bytes of the bucket that its tensors' 2048-bit regions cover; the rest
    is the bucket's padding, which no encoder writes."""
    return sum(_region_bytes(s.numel) for s in b.segments)


def coords_of(b, s) -> torch.Tensor:
    return coord_base(b) + s.bit_off + torch.arange(s.numel, dtype=torch.int64)


def oracle_planes(plan, gs, ms, rr, seed=SEED, step=STEP, beta1=BETA1, cbase=None) -> torch.Tensor:
    """uint8[plan.total_bytes]: ``stochastic_bits_exact`` of every tensor at
    its global coordinates, packed at the tensor's place; region and bucket
    padding 0.  ``cbase``: a coordinate base that replaces every bucket's."""
    out = torch.zeros(plan.total_bytes, dtype=torch.uint8)
    for b in plan.buckets:
        for s in b.segments:
            c = coords_of(b, s) if cbase is None else cbase + s.bit_off + torch.arange(s.numel, dtype=torch.int64)
            bits = ref.stochastic_bits_exact(gs[s.index].cpu(), ms[s.index].cpu(), beta1, rr, c, seed, step)
            o, nb = b.byte_off + s.bit_off // 8, _region_bytes(s.numel)
            out[o:o + nb] = ref.pack_bits(bits, nb * 8)
    return out


def shares(gs, ms, rr, beta1=BETA1):
    """(low clamp, open interval, high clamp) shares of the coordinates, from
    the oracle's fp32 probability before the clamp."""
    u = torch.cat([ref.interp_exact(g, m, beta1).float().reshape(-1) for g, m in zip(gs, ms)])
    rr32 = torch.tensor(rr, dtype=torch.float32)
    raw = (u + rr32) * (torch.tensor(0.5, dtype=torch.float32) / rr32)
    n = raw.numel()
    return (raw <= 0).sum().item() / n, ((raw > 0) & (raw < 1)).sum().item() / n, (raw >= 1).sum().item() / n


# ---------------------------------------------------------------- thresholds
def _ordered(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> int64 keys that increase with the value (+-0 -> 0)."""
    i = x.view(torch.int32).to(torch.int64)
    return torch.where(i >= 0, i, -(i & 0x7FFFFFFF))


def _from_ordered(k: torch.Tensor) -> torch.Tensor:
    i = torch.where(k >= 0, k, (-k) | 0x80000000)
    return torch.where(i >= 1 << 31, i - (1 << 32), i).to(torch.int32).view(torch.float32)


def threshold_case(rr, n=8200, cbase=0, seed=SEED, step=STEP):
    """fp32 (g, m) at beta1 = 1 (u = m exactly, whatever g) that put every
    coordinate on the edge of its own draw: m[i] is the smallest fp32 value
    whose oracle bit is 1 for even i and its predecessor, the largest whose
    bit is 0, for odd i.  The bit is monotone in m, so a bisection over the
    ordered bit patterns finds the edge.  A probability that is one ulp off, a
    draw that keeps one bit less, or ``<=`` for ``<`` flips bits here, where
    random data meets such a difference once in 2^24 coordinates."""
    c = cbase + torch.arange(n, dtype=torch.int64)
    g = torch.randn(n, generator=torch.Generator().manual_seed(11))

    def bit(m):
        return ref.stochastic_bits_exact(g, m, 1.0, rr, c, seed, step)

    lo = _ordered(torch.full((n,), -float(rr) - 1.0))  # p = 0: never 1
    hi = _ordered(torch.full((n,), float(rr) + 1.0))  # p = 1: always 1
    assert not bit(_from_ordered(lo)).any() and bit(_from_ordered(hi)).all()
    while int((hi - lo).max()) > 1:
        mid = (lo + hi) // 2
        up = bit(_from_ordered(mid))
        hi, lo = torch.where(up, mid, hi), torch.where(up, lo, mid)
    odd = (torch.arange(n) & 1).bool()
    m = _from_ordered(torch.where(odd, lo, hi))
    return g, m, ~odd


# ------------------------------------------------------------ special values
def special_values(dtype=torch.bfloat16) -> torch.Tensor:
    """+-0, +-smallest subnormal, +-smallest normal, +-1, +-largest finite,
    +-inf, NaN."""
    fi = torch.finfo(dtype)
    pos = [0.0, fi.smallest_normal * fi.eps, fi.smallest_normal, 1.0, fi.max, float("inf")]
    vals = torch.tensor([v for x in pos for v in (x, -x)] + [float("nan")], dtype=torch.float64).to(dtype)
    assert vals[2].float().item() > 0 and (vals[2].float() / 2).to(dtype).item() == 0  # the smallest subnormal
    return vals


def special_lattice(n=8200, dtype=torch.bfloat16):
    """(p, g, m) of ``n`` elements: g cycles through the 13 special values,
    m through them once per cycle of g, p once per cycle of m -- every (g, m)
    pair 48 times and every (p, g, m) triple at least 3 times in 8200."""
    v = special_values(dtype)
    k = v.numel()
    i = torch.arange(n)
    assert n >= k ** 3
    return v[(i // (k * k)) % k].clone(), v[i % k].clone(), v[(i // k) % k].clone()


def same_bits(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Elementwise: equal bit patterns, or both NaN (any payload)."""
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return (a.contiguous().view(it) == b.contiguous().view(it)) | (torch.isnan(a) & torch.isnan(b))
