"""Shapes and operand generators shared by test_skinny_gemm_gpu.py, test_skinny_gemm_w4_gpu.py and
test_skinny_gemm_cpu.py (the CPU test checks, without a GPU, that every case meets the exactness and tie-share
conditions the GPU tests rely on).  docs/TEST_TOLERANCES.md "Skinny-M GEMM" has the conditions."""
import torch

from numerics import exact_nt, int_operand

from distributed_lion_pytorch_amd.ops import fused

# (M, N, K) of out[M, N] = x[M, K] . w[N, K]^T.  The kernel's units: 16 weight rows per wave, 64 per block, 128 k
# per step (a 64-k last step when K % 128 == 64), 4 steps per chunk, steps split over blocks.
CASES = [
    (1, 16, 64),        # one half step
    (16, 1000, 64),
    (4, 50257, 64),     # huge odd N, one k-step
    (1, 8, 128),        # N below a tile
    (2, 24, 192),       # a full step and a half one
    (3, 40, 256),
    (7, 1003, 128),     # N prime-ish
    (13, 264, 768),     # more than one chunk
    (8, 272, 896),      # Qwen2-0.5B's width
    (16, 136, 1024),
    (5, 24, 2048),
    (9, 50, 4864),
    (16, 16, 14336),    # deep K, forces K splits
]
# every case with K >= 128 asserts this share of exact round-to-even ties on its own reference (the K = 64 sums are
# too small to tie: placement cases only)
MIN_TIE_SHARE = 0.05
TIE_MIN_K = 128
MAX_SPLITS = 32  # csrc/kernels.h kSkinnyMaxSplits


def operands(i, device):
    """x [M, K], w [N, K] of case i: integers in [-7, 7].  Row 0 of x carries k % 7 on top (the kernel permutes k
    inside a step: x and w taking different orders changes the sums) and column 0 of w carries n % 7 (a weight
    row in the wrong output column cannot cancel)."""
    M, N, K = CASES[i]
    return (int_operand((M, K), -7, 7, 100 + i, device, asym="row"),
            int_operand((N, K), -7, 7, 200 + i, device, asym="col"))


def int_bias(i, device):
    """An integer-valued bf16 bias [N] in [-64, 64]: the sum plus it stays exact in fp32."""
    N = CASES[i][1]
    g = torch.Generator().manual_seed(300 + i)
    return torch.randint(-64, 65, (N,), generator=g).to(torch.bfloat16).to(device)


_SUMS = {}


def sum64(i, device):
    """exact_nt of case i's operands, computed once per device."""
    key = (i, str(device))
    if key not in _SUMS:
        _SUMS[key] = exact_nt(*operands(i, device))
    return _SUMS[key]


def split_counts(i):
    """Every forced split count the op accepts for case i that gives a decomposition of its own (the op lowers
    a count to the one that leaves no split empty; counts with the same result are listed once)."""
    M, N, K = CASES[i]
    seen, out = set(), []
    for s in range(1, min(MAX_SPLITS, -(-K // 128)) + 1):
        got = fused.skinny_splits(M, N, K, s)
        if got not in seen:
            seen.add(got)
            out.append(s)
    return out


# ---------------------------------------------------------------------------------------- the 4-bit exact case
W4_CODE = tuple(float(v) for v in range(-8, 8))
W4_SCALES = (0.5, 1.0, 2.0, 4.0)
# the cases of the exact 4-bit check: up to 9 x 50 x 4864 (beyond, at K = 14336, the sums' ties thin out below 0.05)
W4_EXACT = [i for i, (_, _, K) in enumerate(CASES) if K <= 4864]


def w4_exact(i, device):
    """(x, qweight, absmax, code) of case i with an integer codebook: ``code = arange(-8, 8)``, random nibbles,
    ``absmax`` drawn from {0.5, 1, 2, 4}, x integers in [-7, 7].  Every dequantised value (a multiple of 0.5 of
    magnitude <= 32) is exact in bf16."""
    M, N, K = CASES[i]
    g = torch.Generator().manual_seed(400 + i)
    q = torch.randint(0, 256, (N * K // 2,), generator=g, dtype=torch.uint8)
    absmax = torch.tensor(W4_SCALES)[torch.randint(0, 4, (N * K // 64,), generator=g)]
    x = int_operand((M, K), -7, 7, 500 + i, device, asym="row")
    return x, q.to(device), absmax.to(device), torch.tensor(W4_CODE, device=device)


def w4_values(q, absmax, code, N, K, swap_nibbles=False, shift_scale=False):
    """fp64 [N, K] of the store's definition (element 2 j in byte j's high nibble, block b scaled by absmax[b]),
    written out here independently of ops/quant.py; the two flags plant the classic mistakes."""
    hi, lo = (q >> 4).long(), (q & 15).long()
    idx = torch.stack([lo, hi] if swap_nibbles else [hi, lo], dim=1).reshape(-1, 64)
    s = absmax.roll(1) if shift_scale else absmax
    return (code.double()[idx] * s.double()[:, None]).reshape(N, K)
