"""Cases of the wide-rank LoRA kernels (csrc/lora_wide.hip, r in {32, 64, 128}),
shared by test_lora_wide_exact_gpu.py and test_lora_wide_cpu.py.  The operand
generators and the closed forms are lora_exact_cases' own, unchanged; what
differs is the shapes (the edges of the wide kernels' tiles) and the part rule
of lora_cols (fused.lora_cols_parts), under which ``cols_ref`` is evaluated.

Shapes.  lora_rows: a block's 8 waves load NB k-steps of 32 columns each per
pass -- 64 steps (2048 columns) at r = 32 and 32 steps (1024 columns) at r =
64 / 128 -- so K = 1024 / 1056 and 2048 / 2080 bracket the pass boundaries next
to the K of the narrow sweep.  lora_up: a block owns 256 columns (64 per
wave) x 64 tokens; lora_cols: 128 columns (32 per wave) over a row range in
steps of 32 tokens.  N = 128 / 136 and 256 / 264 are the edges of those
blocks, 32 and 480 leave waves without columns."""
import contextlib

import torch

import lora_exact_cases as narrow
from distributed_lion_pytorch_amd.ops import fused
from lora_exact_cases import cols_ref

WIDE_RANKS = [32, 64, 128]

ROWS_K_SWEEP = [32, 256, 288, 1024, 1056, 2048, 2080, 4128, 11008]
UP_N_SWEEP = [32, 128, 136, 256, 264, 480, 512, 520, 768]
# rows = 12801, N = 32 at r = 32: P = 200 and rpp = 65, so parts 197 .. 199 start past the last row
EMPTY_PARTS = (12801, 32)


def wide_parts(rows, N, r):
    """(P, rpp, ranges) by the documented rule (fused.lora_cols_parts)."""
    assert r in WIDE_RANKS
    return fused.lora_cols_parts(rows, N, r)


@contextlib.contextmanager
def _wide_rule(r):
    old = narrow.lora_parts
    narrow.lora_parts = lambda rows, N: wide_parts(rows, N, r)
    try:
        yield
    finally:
        narrow.lora_parts = old


def cols_ref_wide(g, y, a=None, *args, **kwargs):
    """lora_exact_cases.cols_ref with the row ranges of the wide rule at r = y.shape[1]."""
    with _wide_rule(y.shape[1]):
        return cols_ref(g, y, a, *args, **kwargs)


# ---- planted defects of a tiled rank dimension (test_lora_wide_cpu.py)

def drop_tiles(t, dim):
    """``t`` with everything past the first 16 entries of the rank dimension zeroed: a kernel that runs one
    rank tile only."""
    t = t.clone()
    idx = [slice(None)] * t.dim()
    idx[dim] = slice(16, None)
    t[tuple(idx)] = 0
    return t


def swap_tiles(t, dim):
    """``t`` with the first two 16-wide tiles of the rank dimension exchanged."""
    n = t.shape[dim]
    perm = list(range(16, 32)) + list(range(0, 16)) + list(range(32, n))
    return t.index_select(dim, torch.tensor(perm))
