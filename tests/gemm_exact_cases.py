"""Shapes and operand generators shared by test_gemm_exact_gpu.py and
test_gemm_exact_cpu.py (the CPU test checks, without a GPU, that every case
meets the exactness and tie-share conditions the GPU tests rely on)."""
from numerics import int_operand

# every case asserts this share of exact round-to-even ties on its own reference
MIN_TIE_SHARE = 0.05

# (M, N, K): the smallest shapes on both sides of the 128-row wave boundary and
# the 256 tile boundary; K / 128 = 1, 2, 3, 5 covers the single-iteration path
# and both parities of the two-K-tile loop
EDGE_SHAPES = [(1, 8, 128), (127, 72, 128), (129, 264, 256), (255, 248, 384), (256, 256, 128), (257, 520, 128),
               (300, 136, 640), (512, 512, 256)]
# tile order: grids of 7, 7, 9, 27 and 34 blocks, M-groups of 8 + 1 and 8 + 8 + 1
TILE_GRIDS = [(1, 7), (7, 1), (3, 3), (9, 3), (17, 2)]
TILE_SHAPES = [(256 * tm - 100, 256 * tn - 120, 128) for tm, tn in TILE_GRIDS]
NT_SHAPES = EDGE_SHAPES + TILE_SHAPES

# the GELU-forward epilogues scale B by 2^-6: sums stay exact (and ties stay
# ties) but land at |z| ~ 3..8, inside GELU's active range
GELU_SCALE = 2.0 ** -6

# M * lda = 2^31 - 2048 at M = 256: the largest row stride the host check accepts
STRIDE_LD = 2 ** 23 - 8

# (M, N, rows per segment, segments, splits, ldp pad, ldq pad)
TN_CASES = [
    (8, 8, 128, 1, 1, 0, 0),        # the min(., M - 8) / min(., N - 8) clamps are 0
    (264, 776, 128, 2, 1, 0, 0),
    (264, 776, 128, 2, 2, 0, 0),
    (256, 256, 128, 16, 1, 0, 0),   # one pair per segment: every advance() crosses a segment
    (256, 256, 128, 16, 3, 0, 0),
    (256, 256, 128, 16, 16, 0, 0),  # splits == kpairs
    (520, 136, 256, 3, 6, 0, 0),    # one pair per split
    (520, 136, 256, 3, 4, 0, 0),    # uneven splits (1, 2, 1, 2 pairs); split 3 starts on a segment boundary
    (776, 264, 512, 2, 3, 8, 16),   # row strides > width
]

GELU_UNFUSED_ROWS = [1, 5, 300]
GELU_UNFUSED_N = [8, 520, 1024 * 8, 1025 * 8]  # 1025 groups of 8: two groups per thread

def nt_operands(M, N, K, device, scale=1.0):
    """a [M, K], b [N, K]: integers in [-7, 7], column 0 of each made asymmetric; b times ``scale``."""
    seed = 1000003 * M + 1009 * N + K
    a = int_operand((M, K), -7, 7, seed, device, asym="col")
    b = int_operand((N, K), -7, 7, seed + 1, device, asym="col", scale=scale)
    return a, b


def tn_operands(M, N, rows, nseg, device):
    """P [rows, M] x nseg, Q [rows, N] x nseg: integers in [-7, 7], row 0 of each segment asymmetric."""
    seed = 1000003 * M + 1009 * N + 7 * rows + nseg
    P = [int_operand((rows, M), -7, 7, seed + 2 * i, device, asym="row") for i in range(nseg)]
    Q = [int_operand((rows, N), -7, 7, seed + 2 * i + 1, device, asym="row") for i in range(nseg)]
    return P, Q


def tn_split_rows(rows, nseg, splits):
    """Row range [p0 * 128, p1 * 128) of every split, p = floor(z * kpairs / splits)."""
    kpairs = nseg * rows // 128
    return [(z * kpairs // splits * 128, (z + 1) * kpairs // splits * 128) for z in range(splits)]
