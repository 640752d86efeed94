"""Exact-arithmetic conformance of the NT GEMM and its nine epilogues
(csrc/gemm.hip), the weight-gradient GEMM (csrc/gemm_tn.hip) and the unfused
bias+GELU kernels (csrc/elementwise_kernels.hip).

Small-integer operands make every product and partial sum exact in fp32, so
the plain / bias / multiply epilogues and the TN kernel are compared bit for
bit with ONE deterministic rounding of an exactly known number; 5 % or more of
those numbers are exact round-to-even ties (asserted per case), so the rounding
mode itself is under test.  The GELU epilogues are judged elementwise against
fp64 closed forms to half a bf16 ulp plus the error of a plain fp32 evaluation
of the same form (numerics.assert_rounded / eval_floor), the bias-gradient
partials slab by slab against the column sums of the kernel's own output.
docs/TEST_TOLERANCES.md "GEMM" has the derivations and the measured ratios;
gemm_exact_cases.py the shapes."""
import functools

import pytest
import torch

from distributed_lion_pytorch_amd.ops import hip

from gemm_exact_cases import (EDGE_SHAPES, GELU_SCALE, GELU_UNFUSED_N, GELU_UNFUSED_ROWS, MIN_TIE_SHARE, NT_SHAPES,
                              STRIDE_LD, TILE_SHAPES, TN_CASES, nt_operands, tn_operands, tn_split_rows)
from numerics import (GEMM_SLAB, assert_bits, assert_col_partials, assert_rounded, eval_floor, exact_nt, exact_tn, expect_nt,
                      gelu64, gelu_form, gelu_grad64, gelu_grad_form, gemm_slabs, int_operand, strided_rows, tie_share)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN = float("nan")


def _ops():
    hip.require()
    return hip.ops()


@functools.lru_cache(maxsize=None)
def _nt(M, N, K, scale=1.0):
    """(a, b, exact fp64 product) on the GPU, shared by the tests of one shape and never written."""
    a, b = nt_operands(M, N, K, "cuda", scale)
    s = exact_nt(a, b)
    share = tie_share(s)
    print(f"[ties] NT {M}x{N}x{K}: {share:.3f}")
    assert share >= MIN_TIE_SHARE, f"tie share {share:.3f} of {M}x{N}x{K}: the case no longer exercises the rounding"
    return a, b, s


def _padded(t, pad, fill=NAN):
    """t as the leading columns of a wider, ``fill``-filled buffer (row stride = width + pad)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, device=t.device, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _inner(t, pad):
    """t as an inner column slice [8 : 8 + n] of a NaN-filled buffer of row stride n + pad."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), NAN, device=t.device, dtype=t.dtype)
    v = buf[:, 8:8 + t.shape[1]]
    v.copy_(t)
    return v


def _rand_bf16(shape, seed, lo=None, hi=None, std=1.0):
    g = torch.Generator().manual_seed(seed)
    if lo is None:
        t = torch.randn(shape, generator=g) * std
    else:
        t = torch.rand(shape, generator=g) * (hi - lo) + lo
    return t.to(BF16).cuda()


# --------------------------------------------------------------------------- NT: plain / bias (EPI 0 / 1)
@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_nt_plain_and_bias_bit_exact(M, N, K):
    ops = _ops()
    a, b, s = _nt(M, N, K)
    ap, bp = _padded(a, 8), _padded(b, 24)  # lda = K + 8, ldb = K + 24; the padding is NaN
    biases = {"none": None,
              "integer": int_operand((1, N), -64, 64, 7 * M + N, "cuda", asym=None)[0].contiguous(),
              "random": _rand_bf16((N,), 11 * M + N, std=4.0)}
    for kind, bias in biases.items():
        full = torch.full((M + 3, N + 8), NAN, device="cuda", dtype=BF16)  # ldc = N + 8
        ops.gemm_nt_out(ap, bp, bias, full[:M, :N])
        name = f"EPI {0 if bias is None else 1} ({kind} bias) {M}x{N}x{K}"
        inside = torch.zeros_like(full, dtype=torch.bool)
        inside[:M, :N] = True
        assert bool(full[~inside].isnan().all()), f"{name}: wrote outside [0:M, 0:N]"
        assert not bool(full[:M, :N].isnan().any()), f"{name}: NaN / unwritten elements inside [0:M, 0:N]"
        assert_bits(full[:M, :N], expect_nt(s, bias), name)
        # the operand padding is never read: the contiguous call gives the same bits
        assert_bits(ops.gemm_nt(a, b, bias), full[:M, :N].contiguous(), name + " contiguous")


# --------------------------------------------------------------------------- NT: GELU forward (EPI 2 / 3, 6 / 7)
def _gelu_case(M, N, K):
    """Operands whose exact sums are multiples of 2^-6 of magnitude ~3..8: u = z + b
    spans GELU's active range instead of sitting in the saturated tails."""
    a, b, s = _nt(M, N, K, GELU_SCALE)
    bias = _rand_bf16((N,), 13 * M + N)
    z = expect_nt(s)
    return a, b, bias, z, z.float() + bias.float()


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("M,N,K", EDGE_SHAPES)
def test_nt_gelu_epilogue(M, N, K, exact):
    ops = _ops()
    a, b, bias, z_exp, u = _gelu_case(M, N, K)
    h, z = ops.gemm_nt_gelu(a, b, bias, exact)
    name = f"EPI {3 if exact else 2} {M}x{N}x{K}"
    assert_bits(z, z_exp, name + " z")
    assert_bits(h, ops.bias_gelu_fwd(z_exp, bias, exact), name + " h vs bias_gelu_fwd")
    assert_rounded(h, gelu64(u, exact), eval_floor(lambda t: gelu_form(t, exact), u), name + " h")


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("M,N,K", EDGE_SHAPES)
def test_nt_gelu_derivative_store_epilogue(M, N, K, exact):
    ops = _ops()
    a, b, bias, z_exp, u = _gelu_case(M, N, K)
    h, d = ops.gemm_nt_gelu_d(a, b, bias, exact)
    name = f"EPI {7 if exact else 6} {M}x{N}x{K}"
    assert_bits(h, ops.bias_gelu_fwd(z_exp, bias, exact), name + " h vs bias_gelu_fwd")
    assert_rounded(h, gelu64(u, exact), eval_floor(lambda t: gelu_form(t, exact), u), name + " h")
    # the tanh derivative crosses zero near u = -0.75: there the floor carries the element
    assert_rounded(d, gelu_grad64(u, exact), eval_floor(lambda t: gelu_grad_form(t, exact), u), name + " d")


# --------------------------------------------------------------------------- NT: multiply by a stored derivative (EPI 8)
@pytest.mark.parametrize("kind", ["integer", "random"])
@pytest.mark.parametrize("M,N,K", EDGE_SHAPES + TILE_SHAPES)
def test_nt_dmul_epilogue(M, N, K, kind):
    ops = _ops()
    a, b, s = _nt(M, N, K)
    if kind == "integer":
        d = int_operand((M, N), -2, 2, 17 * M + N, "cuda", asym=None)
    else:
        d = _rand_bf16((M, N), 19 * M + N)
    dz, part = ops.gemm_nt_dmul(a, b, _inner(d, 16))  # ldaux = N + 16
    name = f"EPI 8 ({kind} d) {M}x{N}x{K}"
    # bf16 x bf16 is exact in fp32: one rounding
    assert_bits(dz, (expect_nt(s).float() * d.float()).to(BF16), name + " dz")
    assert_col_partials(part, dz, gemm_slabs(M), GEMM_SLAB, exact=kind == "integer", name=name + " part")


# --------------------------------------------------------------------------- NT: DGELU (EPI 4 / 5)
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("M,N,K", EDGE_SHAPES + TILE_SHAPES)
def test_nt_dgelu_epilogue(M, N, K, exact):
    ops = _ops()
    a, b, s = _nt(M, N, K)
    bias = _rand_bf16((N,), 23 * M + N)
    z = _rand_bf16((M, N), 29 * M + N, lo=-6.0, hi=6.0)
    dz, part = ops.gemm_nt_dgelu(a, b, bias, _inner(z, 16), exact)
    name = f"EPI {5 if exact else 4} {M}x{N}x{K}"
    g = expect_nt(s).double()
    u = z.float() + bias.float()
    floor = g.abs() * eval_floor(lambda t: gelu_grad_form(t, exact), u)
    assert_rounded(dz, g * gelu_grad64(u, exact), floor, name + " dz")
    assert_col_partials(part, dz, gemm_slabs(M), GEMM_SLAB, name=name + " part")
    # common.h: the DGELU epilogue and the unfused backward share gelu_grad, bit for bit
    dz_unfused = ops.bias_gelu_bwd(ops.gemm_nt(a, b, None), z, bias, exact, 7)[0]
    assert_bits(dz, dz_unfused, name + " dz vs bias_gelu_bwd")


# --------------------------------------------------------------------------- NT: the largest accepted stride
def test_nt_largest_accepted_stride():
    """M * lda = 2^31 - 2048: the last row's 32-bit lane byte offset is just
    below 2^32.  One more row must be refused on the host."""
    ops = _ops()
    ld, K = STRIDE_LD, 128
    if torch.cuda.mem_get_info()[0] < 6 * 2 ** 30:
        pytest.skip("needs 6 GiB of free GPU memory")
    buf = torch.empty(257 * ld, device="cuda", dtype=BF16).view(257, ld)  # only the slices below are ever touched
    big = buf[:256, :K]
    assert big.shape[0] * big.stride(0) == 2 ** 31 - 2048
    small_m, other = nt_operands(256, 264, K, "cuda")[0], nt_operands(300, 264, K, "cuda")[1]
    big.copy_(small_m)
    # as A
    assert_bits(ops.gemm_nt(big, other, None), ops.gemm_nt(small_m, other, None), "A with lda = 2^23 - 8")
    # as B (N = 256 rows of that stride)
    a300 = nt_operands(300, 264, K, "cuda")[0]
    assert_bits(ops.gemm_nt(a300, big, None), ops.gemm_nt(a300, small_m, None), "B with ldb = 2^23 - 8")
    assert_bits(ops.gemm_nt(a300, small_m, None), expect_nt(exact_nt(a300, small_m)), "contiguous reference")
    with pytest.raises(RuntimeError):  # M = 257: refused before anything is launched
        ops.gemm_nt(buf[:, :K], other, None)


# --------------------------------------------------------------------------- TN
@pytest.mark.parametrize("M,N,rows,nseg,splits,ldp_pad,ldq_pad", TN_CASES)
def test_tn_bit_exact(M, N, rows, nseg, splits, ldp_pad, ldq_pad):
    ops = _ops()
    P, Q = tn_operands(M, N, rows, nseg, "cuda")
    Pc, Qc = torch.cat(P), torch.cat(Q)
    s = exact_tn(P, Q)
    if ldp_pad or ldq_pad:
        P, Q = [_padded(p, ldp_pad) for p in P], [_padded(q, ldq_pad) for q in Q]
    name = f"TN {M}x{N} rows {rows} x {nseg} splits {splits}"
    out = ops.gemm_tn(P, Q, splits)
    assert out.shape == (splits, M, N) and out.dtype == torch.float32
    # every slice is the exact sum over its own rows: each row is counted exactly once
    slices = []
    for z, (r0, r1) in enumerate(tn_split_rows(rows, nseg, splits)):
        exp = exact_tn(Pc[r0:r1], Qc[r0:r1])
        slices.append(exp)
        assert_bits(out[z], exp.float(), f"{name} slice {z} rows [{r0}, {r1})")
    assert torch.equal(torch.stack(slices).sum(0), s)
    # fp32 accumulate onto an integer-valued accumulator
    g = torch.Generator().manual_seed(M + N + splits)
    old = torch.randint(-1000, 1001, (splits, M, N), generator=g).float().cuda()
    acc = old.clone()
    ops.gemm_tn_(P, Q, acc, True)
    assert_bits(acc, (old.double() + torch.stack(slices)).float(), name + " fp32 accumulate")
    # unsplit bf16 output, from NaN; accumulate onto an integer-valued bf16 gradient
    share = tie_share(s)
    print(f"[ties] {name}: {share:.3f}")
    assert share >= MIN_TIE_SHARE, f"{name}: tie share {share:.3f}"
    outb = torch.full((M, N), NAN, device="cuda", dtype=BF16)
    ops.gemm_tn_(P, Q, outb, False)
    assert_bits(outb, expect_nt(s), name + " bf16")
    oldb = int_operand((M, N), -64, 64, M + 3 * N, "cuda", asym=None) * 2 + 1  # odd: a sentinel no sum leaves in place
    accb = oldb.clone()
    ops.gemm_tn_(P, Q, accb, True)
    assert_bits(accb, (s.float() + oldb.float()).to(BF16), name + " bf16 accumulate")


# --------------------------------------------------------------------------- unfused bias + GELU
def _gelu_inputs(rows, N):
    z = _rand_bf16((rows, N), 31 * rows + N, lo=-8.0, hi=8.0)
    b = _rand_bf16((N,), 37 * rows + N, lo=-4.0, hi=4.0)
    return z, b, z.float() + b.float()  # u in [-12, 12]: both saturated tails


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("N", GELU_UNFUSED_N)
@pytest.mark.parametrize("rows", GELU_UNFUSED_ROWS)
def test_bias_gelu_fwd(rows, N, exact):
    ops = _ops()
    z, b, u = _gelu_inputs(rows, N)
    h = ops.bias_gelu_fwd(z, b, exact)
    assert_rounded(h, gelu64(u, exact), eval_floor(lambda t: gelu_form(t, exact), u),
                   f"bias_gelu_fwd {'erf' if exact else 'tanh'} {rows}x{N}")


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("N", GELU_UNFUSED_N)
@pytest.mark.parametrize("rows", GELU_UNFUSED_ROWS)
def test_bias_gelu_bwd(rows, N, exact):
    ops = _ops()
    z, b, u = _gelu_inputs(rows, N)
    dh = _rand_bf16((rows, N), 41 * rows + N)
    ref = dh.double() * gelu_grad64(u, exact)
    floor = dh.double().abs() * eval_floor(lambda t: gelu_grad_form(t, exact), u)
    first = None
    for parts in (1, 7, rows + 3):  # rows + 3: three blocks walk no row
        dz, part = ops.bias_gelu_bwd(dh, z, b, exact, parts)
        name = f"bias_gelu_bwd {'erf' if exact else 'tanh'} {rows}x{N} parts {parts}"
        assert_rounded(dz, ref, floor, name + " dz")
        assert_col_partials(part, dz, strided_rows(rows, parts), name=name + " part")
        if first is None:
            first = dz
        assert_bits(dz, first, name + " dz vs parts 1")
