"""Cases, operand generators and closed forms shared by test_lora_exact_gpu.py
and test_lora_exact_cpu.py (csrc/lora.hip; docs/TEST_TOLERANCES.md "LoRA and
4-bit").

The ``*_ref`` functions are the kernels' documented arithmetic in plain
PyTorch on the CPU: fp64 sums (exact for the integer operands, which
``exact=True`` asserts) followed by the kernels' fp32 / bf16 roundings.  The
GPU tests compare the kernels with them bit for bit; the CPU test plants
defects in them (``defect=...``) and shows that the same comparison rejects
every one."""
import torch

from distributed_lion_pytorch_amd.ops import fused
from numerics import _assert_exact, _unit, drop_consts, int_operand, lora_parts, part_sums64

BF16 = torch.bfloat16
RANKS = [8, 16]
# every case designated for ties asserts this share of exact round-to-even ties, on
# the adapter term and on the sum (the CPU test shows the generators stay above it)
MIN_TIE_SHARE = 0.05

ROWS_M = 33
ROWS_K_SWEEP = [32, 256, 288, 4096, 4128, 11008]  # 1, 8, 9, 128, 129, 344 k-steps: see the GPU test
ROWS_K = 256
ROWS_M_SWEEP = [1, 15, 16, 17, 1027]
DROPS = [0.0, 0.5, 0.75]

UP_M = 67
UP_N_SWEEP = [32, 480, 512, 520, 768]
UP_N = 520
UP_M_SWEEP = [1, 5, 16, 17, 100, 1027]
EMPTY_PARTS = (8200, 32)  # P = 512, rpp = 17: parts 483 .. 511 have no rows

# (M, K, N) of the row-wise cases at realistic data
RANDN_SHAPES = [(1027, 512, 768), (67, 11008, 512), (130, 256, 4096)]
RANDN_P, RANDN_S = 0.1, 1.7

SENTINEL = 96.0  # fills the columns around a strided operand


def case_scale(*key) -> float:
    """2.0 or 0.5, alternating with the case."""
    return 2.0 if sum(int(k) for k in key) % 2 == 0 else 0.5


def _seed(*key) -> int:
    s = 17
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return s


def rows_operands(M, K, r, device="cpu"):
    """x [M, K] and a [r, K]: integers in [-3, 3], column 0 of each made asymmetric."""
    x = int_operand((M, K), -3, 3, _seed(1, M, K, r), device, asym="col")
    a = int_operand((r, K), -3, 3, _seed(2, M, K, r), device, asym="col")
    return x, a


def up_operands(M, N, r, device="cpu"):
    """o [M, N] (integers in [-200, 200]) and b [N, r] (in [-7, 7]) for lora_up, dout [M, N] (in [-7, 7])
    for lora_cols mode 0; column 0 of each asymmetric.  u comes from rows_operands(M, ROWS_K, r)."""
    o = int_operand((M, N), -200, 200, _seed(3, M, N, r), device, asym="col")
    b = int_operand((N, r), -7, 7, _seed(4, M, N, r), device, asym="col")
    dout = int_operand((M, N), -7, 7, _seed(5, M, N, r), device, asym="col")
    return o, b, dout


def dx_operands(M, N, r, device="cpu", nout=32):
    """lora_cols mode 1 at width N: x [M, N] (integers in [-3, 3]), a [r, N] in [1, 7], and the operands of
    its du = lora_rows(dout, b^T): dout [M, nout] in [1, 5], b [nout, r] in [1, 3].  du and a are strictly
    positive, so dx is non-zero exactly where the mask keeps."""
    x = int_operand((M, N), -3, 3, _seed(6, M, N, r), device, asym="col")
    a = int_operand((r, N), 1, 7, _seed(7, M, N, r), device, asym="col")
    dout = int_operand((M, nout), 1, 5, _seed(8, M, N, r), device, asym="col")
    b = int_operand((nout, r), 1, 3, _seed(9, M, N, r), device, asym="col")
    return x, a, dout, b


def strided(t, left=8, right=16, fill=SENTINEL):
    """``t`` as a column slice of a wider tensor whose other columns hold ``fill``."""
    wide = torch.full((t.shape[0], left + t.shape[1] + right), fill, dtype=t.dtype, device=t.device)
    wide[:, left:left + t.shape[1]] = t
    v = wide[:, left:left + t.shape[1]]
    assert not v.is_contiguous() or t.shape[0] == 1
    return v


def keep_mask(M, K, p, seed, defect=None, ld=None):
    """The host's keep mask [M, K] (all ones when the threshold is 0)."""
    th, _ = drop_consts(p)
    if th == 0:
        return torch.ones(M, K, dtype=torch.bool)
    if defect == "mask_stride":  # the flat index t * ld + c of a strided operand instead of t * K + c
        return fused.norm_dropout_keep(M, ld, p, seed)[:, :K].clone()
    keep = fused.norm_dropout_keep(M, K, p, seed).clone()
    if defect == "flip_bit":
        keep[M // 2, K // 3] ^= True
    return keep


def _rne(x32, defect=None):
    """fp32 -> bf16, round to nearest even (``half_up``: ties away from zero)."""
    if defect == "half_up":
        bits = x32.contiguous().view(torch.int32)
        return ((bits + 0x8000) & ~0xFFFF).view(torch.float32).to(BF16)
    return x32.to(BF16)


def _f32(s64, what, exact):
    """The fp64 sum as the fp32 the kernel holds; a zero sum is +0 (accumulators start at +0)."""
    s32 = s64.float() + 0.0
    if exact:
        assert torch.equal(s32.double(), s64), f"{what}: sum not exact in fp32"
    return s32


def rows_ref(x, a, scale, p=0.0, seed=0, defect=None, ld=None, exact=True):
    """u = bf16(fp32(sum_k xd[t, k] a[j, k]) * scale), xd = bf16(x * inv_keep) where kept and +0 where dropped."""
    x, a = x.detach().cpu(), a.detach().cpu()
    M, K = x.shape
    _, inv = drop_consts(p)
    keep = keep_mask(M, K, p, seed, defect, ld)
    xd = torch.where(keep, (x.float() * inv).to(BF16), torch.zeros((), dtype=BF16)).double()
    if defect == "k_tail":  # the outer loop runs once: k-steps >= 8 * 16 are lost
        xd[:, 4096:] = 0
    a64 = a.double()
    if exact:
        _assert_exact(xd.abs() @ a64.abs().t(), _unit(xd, a64), "rows_ref")
    return _rne(_f32(xd @ a64.t(), "rows_ref", exact) * scale, defect)


def up_ref(o, u, b, s, defect=None, exact=True):
    """out = bf16(fp32(o) + fp32(bf16(fp32(sum_j u[t, j] b[n, j]) * s))): two roundings.  Returns (out, the
    adapter term before its rounding, the sum before its rounding), the last two in fp64."""
    o, u, b = o.detach().cpu(), u.detach().cpu(), b.detach().cpu()
    u64, b64 = u.double(), b.double()
    if exact:
        _assert_exact(u64.abs() @ b64.abs().t(), _unit(u64, b64), "up_ref")
    inner = _f32(u64 @ b64.t(), "up_ref", exact) * s
    ad = inner if defect == "no_inner_rounding" else _rne(inner, defect).float()
    total = o.float() + ad
    if exact:
        assert torch.equal(total.double(), o.double() + ad.double()), "up_ref: o + adapter not exact in fp32"
    return _rne(total, defect), inner.double(), total.double()


def cols_ref(g, y, a=None, yscale=1.0, p=0.0, seed=0, defect=None, ld=None, exact=True):
    """lora_cols.  Without a (mode 0): part [P, N, R] = yscale * sum_t g[t, n] y[t, j] per part, dx None.
    With a [R, N] (mode 1): part [P, R, N] = sum_t y[t, j] g'[t, n], g' = g * inv_keep where kept (not
    rounded), and dx[t, n] = bf16(inv_keep * sum_j y[t, j] a[j, n]) where kept, +0 where dropped."""
    g, y = g.detach().cpu(), y.detach().cpu()
    M, N = g.shape
    P, rpp, ranges = lora_parts(M, N)
    dx = None
    g64, y64 = g.double(), y.double()
    if a is not None:
        _, inv = drop_consts(p)
        keep = keep_mask(M, N, p, seed, defect, ld)
        g64 = torch.where(keep, g64 * inv, torch.zeros((), dtype=torch.float64))
        a64 = a.detach().cpu().double()
        if exact:
            _assert_exact(y64.abs() @ a64.abs(), _unit(y64, a64), "cols_ref dx")
        d = _f32(y64 @ a64, "cols_ref dx", exact) * inv
        dx = torch.where(keep, _rne(d, defect), torch.zeros((), dtype=BF16))
    layout = "nr" if a is None else "rn"
    if defect == "swap_layout":
        layout = "rn" if a is None else "nr"
    s, mag = part_sums64(g64, y64, ranges, layout)
    if defect == "tail_twice":  # the last (partly zero-filled) batch of 4 rows of part 0 enters twice
        r0, r1 = ranges[0]
        t0 = r0 + (r1 - r0 - 1) // 4 * 4
        s2, _ = part_sums64(g64[t0:r1], y64[t0:r1], [(0, r1 - t0)], layout)
        s[0] += s2[0]
    if exact:
        _assert_exact(mag, _unit(g64, y64), "cols_ref part")
    part = _f32(s * yscale, "cols_ref part", exact)
    if defect == "swap_layout":
        part = part.contiguous().view(P, N, -1) if a is None else part.contiguous().view(P, -1, N)
    return part, dx


# ---- the forward mask, read back element by element through lora_rows itself

def probe_windows(K, r):
    return (K + 8 * r - 1) // (8 * r)


def probe_weights(K, r, w, device="cpu"):
    """a [r, K]: a[j, w 8r + 8 j + b] = 2^b, zero elsewhere.  With x = 1, u[t, j] / (scale inv_keep) is the
    8-bit word of the keep bits of columns w 8r + 8 j .. + 7 of row t -- exact in bf16 (8 significant bits)."""
    a = torch.zeros(r, K)
    for j in range(r):
        for b in range(8):
            k = w * 8 * r + 8 * j + b
            if k < K:
                a[j, k] = 2.0 ** b
    return a.to(BF16).to(device)


def probe_decode(us, K, r, scale, p):
    """The keep mask [M, K] from the u of every window (a list of [M, r] tensors)."""
    _, inv = drop_consts(p)
    M = us[0].shape[0]
    keep = torch.zeros(M, probe_windows(K, r) * 8 * r, dtype=torch.bool)
    for w, u in enumerate(us):
        word = u.detach().cpu().double() / (scale * inv)
        assert bool(((word == word.floor()) & (word >= 0) & (word < 256)).all()), "probe: u is not an 8-bit word"
        word = word.long()
        for b in range(8):
            keep[:, w * 8 * r + b:(w + 1) * 8 * r:8] = ((word >> b) & 1).bool()
    assert not bool(keep[:, K:].any())
    return keep[:, :K]


# ---- fp64 references and row-wise bounds of the whole op (ops/fused._LoraAdd), for test_lora_gpu.py

def chain_bounds(x, o, a, b, dout, s, p, seed):
    """fp64 (ref, floor) of out, dx, dA and dB of out = o + s (drop(x) A^T) B^T, each result one bf16 rounding of
    a value within ``floor`` of ref (numerics.assert_rounded); for out the floor includes the half ulp of the
    adapter term.  The op rounds two intermediates to bf16, u = drop(x) A^T and du = s dout B; their errors
    e_u = half_ulp(u) + K 2^-24 sum |xd a| and e_du = half_ulp(du) + N 2^-24 s sum |dout b| enter every result
    linearly and are propagated with the magnitudes of the other operand (worst case, no cancellation), next
    to the n 2^-24 sum |terms| of the result's own fp32 sum (docs/TEST_TOLERANCES.md "LoRA and 4-bit")."""
    from numerics import SUM_EPS, bf16_half_ulp

    x, o, a, b, dout = (t.detach().cpu() for t in (x, o, a, b, dout))
    M, K = x.shape
    N, r = b.shape
    _, inv = drop_consts(p)
    keep = keep_mask(M, K, p, seed)
    zero = torch.zeros((), dtype=torch.float64)
    xd = torch.where(keep, (x.float() * inv).to(BF16).double(), zero)   # the forward's bf16 drop(x)
    xs = torch.where(keep, x.double() * inv, zero)                      # the dA sum's unrounded one
    a64, b64, d64 = a.double(), b.double(), dout.double()
    u = xd @ a64.t()
    e_u = bf16_half_ulp(u) + K * SUM_EPS * (xd.abs() @ a64.abs().t())
    du = s * (d64 @ b64)
    e_du = bf16_half_ulp(du) + N * SUM_EPS * s * (d64.abs() @ b64.abs())
    inner = s * (u @ b64.t())
    e_inner = s * (e_u @ b64.abs().t()) + r * SUM_EPS * s * (u.abs() @ b64.abs().t())
    return {
        "out": (o.double() + inner, bf16_half_ulp(inner) + e_inner),
        "dx": (torch.where(keep, inv * (du @ a64), zero),
               torch.where(keep, inv * (e_du @ a64.abs()) + r * SUM_EPS * inv * (du.abs() @ a64.abs()), zero)),
        "dA": (du.t() @ xs, e_du.t() @ xs.abs() + M * SUM_EPS * (du.abs().t() @ xs.abs())),
        "dB": (s * (d64.t() @ u), s * (d64.abs().t() @ e_u) + M * SUM_EPS * s * (d64.abs().t() @ u.abs())),
    }
