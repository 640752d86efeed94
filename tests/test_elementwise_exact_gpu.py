"""Exact-arithmetic and elementwise fp64 tests of the SwiGLU, RoPE, partial-sum
and column-sum kernels (csrc/elementwise_kernels.hip), one raw op at a time.

RoPE, the partial sums in every form and on every route and the column sums
run on integer operands and are compared bit for bit with one rounding of the
exact value; SwiGLU is judged elementwise against fp64 with a floor counted
from the kernel's fp32 roundings (docs/TEST_TOLERANCES.md "Norm, SwiGLU, RoPE
and partial sums").  The cases and checks live in elementwise_exact_cases.py;
test_elementwise_exact_cpu.py runs the same ones on fp32 emulations with
planted defects."""
import pytest

import elementwise_exact_cases as ec
from distributed_lion_pytorch_amd.ops import hip

pytestmark = pytest.mark.gpu

LAYOUTS = ["contiguous", "halves"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("F", ec.SWIGLU_F)
@pytest.mark.parametrize("rows", ec.SWIGLU_ROWS)
def test_swiglu(rows, F, layout, cuda):
    """h, dg, du of swiglu_fwd / swiglu_bwd / swiglu_bwd_fused against fp64, gates at 0, +-2^-10, the zero of
    silu', +-20, +-60, -87, -89, -200 among 3 randn; every output finite."""
    hip.require()
    w = ec.check_swiglu(hip.ops(), rows, F, layout, cuda)
    print("worst err / bound (h, dg, du): " + " ".join(f"{v:.3f}" for v in w))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows,F", ec.SWIGLU_T)
def test_swiglu_transposing(rows, F, layout, cuda):
    """swiglu_fwd_t / swiglu_bwd_fused_t against fp64, row-major and transposed, and the two copies bit for bit."""
    hip.require()
    ec.check_swiglu_t(hip.ops(), rows, F, layout, cuda)


@pytest.mark.parametrize("D", ec.ROPE_D)
@pytest.mark.parametrize("H", ec.ROPE_H)
def test_rope(H, D, cuda):
    """rope / rope_ forward and inverse with independent, asymmetric tables: bit for bit, contiguous, token-strided
    and in place between sentinels; the adjoint identity; the unit tables."""
    hip.require()
    print(f"min tie share {ec.check_rope(hip.ops(), H, D, cuda):.3f}")


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("S,n", ec.PARTIAL_SHAPES)
def test_sum_partials(S, n, strided, cuda):
    """plain, _acc_, _scaled_ (0.5 and 4, with and without accumulation) and the one-stack _multi_ form: bit for bit."""
    hip.require()
    route, share = ec.check_partials(hip.ops(), S, n, strided, cuda)
    print(f"route {route}, min tie share {share:.3f}")


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("heights,n", ec.MULTI_CASES)
def test_sum_partials_multi(heights, n, strided, cuda):
    """sum_partials_multi_ over stacks of unequal height, on the split route and on the multi kernel: bit for bit."""
    hip.require()
    route, share = ec.check_partials_multi(hip.ops(), heights, n, strided, cuda)
    print(f"route {route}, min tie share {share:.3f}")


@pytest.mark.parametrize("rows,parts", ec.COLSUM_ROWS_PARTS)
@pytest.mark.parametrize("N", ec.COLSUM_N)
def test_colsum_partials(N, rows, parts, cuda):
    """Every partial row of colsum_partials is the exact sum of its strided row set."""
    hip.require()
    ec.check_colsum(hip.ops().colsum_partials, N, rows, parts, cuda)
