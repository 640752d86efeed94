"""Exact-arithmetic and row-wise fp64 tests of the fused residual + dropout +
LayerNorm / RMSNorm kernels (csrc/norm_kernels.hip), one raw op at a time.

With integer operands the residual store, the row mean, the backward's dx / dy
and every per-block partial sum have an expected value that is one
deterministic rounding, so they are compared bit for bit; rstd, h and the randn
rows are judged against fp64 with bounds derived from the number of fp32
roundings (docs/TEST_TOLERANCES.md "Norm, SwiGLU, RoPE and partial sums").
The cases, generators and checks live in norm_exact_cases.py;
test_norm_exact_cpu.py runs the same ones on fp32 emulations with planted
defects."""
import pytest

import norm_exact_cases as nc
from distributed_lion_pytorch_amd.ops import hip

pytestmark = pytest.mark.gpu


def _fwd(*a):
    return hip.ops().add_norm_fwd(*a)


def _bwd(*a):
    return hip.ops().add_norm_bwd(*a)


@pytest.mark.parametrize("C,rms,rows", nc.FWD_CASES)
def test_fwd_residual_mean_and_output(C, rms, rows, cuda):
    """(a) + (c): xo = bf16(x + keep inv_keep (y + bias)) bit for bit with at least 10 % ties, dropped positions
    untouched, mean = fp32(sum) * fp32(1 / C) bit for bit (0 for RMS), h within half a bf16 ulp + 2^-21."""
    hip.require()
    print(f"min tie share {nc.run_fwd_residual(_fwd, C, rms, rows, cuda):.3f}")


@pytest.mark.parametrize("C,rms", nc.CASES)
def test_fwd_exact_statistics(C, rms, cuda):
    """(b): rows of mean 0, 1, -2, 4, 8 whose sum of squared deviations is an exact integer: mean exact, rstd
    within relative 2^-21 of fp64, eps = 1e-5 and 0."""
    hip.require()
    print(f"worst |rstd - ref| / (2^-21 ref): {nc.run_fwd_stats(_fwd, C, rms, cuda):.3f}")


@pytest.mark.parametrize("C,rms", nc.CASES)
def test_fwd_randn_rows_far_from_zero(C, rms, cuda):
    """(d): randn rows whose mean is 3 to 5 standard deviations from zero: mean and rstd within the order-free
    fp32 sum bound of fp64."""
    hip.require()
    wm, wr = nc.run_fwd_offset(_fwd, C, rms, cuda)
    print(f"worst err / bound: mean {wm:.3f} rstd {wr:.3f}")


@pytest.mark.parametrize("C,rms", nc.CASES)
def test_bwd_exact(C, rms, cuda):
    """dx and dy bit for bit with the closed form dx = bf16(dxo_in + rstd w), every block's dgamma / dbeta / dbias
    partial row bit for bit, with parts = 1, an uneven split and more blocks than row groups."""
    hip.require()
    print(f"min tie share of dx {nc.run_bwd_exact(_bwd, C, rms, cuda):.3f}")


@pytest.mark.parametrize("C,rms", nc.CASES)
def test_bwd_randn(C, rms, cuda):
    """randn rows: dx and dy within half a bf16 ulp + the propagated fp32 sum bounds of fp64 fed the same statistics."""
    hip.require()
    print(f"worst err / bound of dx {nc.run_bwd_randn(_bwd, C, rms, cuda):.3f}")
