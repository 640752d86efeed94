"""test_lora_exact_gpu.py's generators, closed forms and criteria without a GPU:
every parametrised case meets the exactness and tie-share conditions, the part
ranges follow the documented rule, the mask probe reads every keep bit, and
defects planted in the closed forms (the kernels' arithmetic in PyTorch) are
rejected by the same bit comparison the GPU tests apply.  For each defect the
old criterion of test_lora_gpu.py -- max |got - ref| / max |ref| below 1e-2
(output) or 2e-2 (gradients) -- is evaluated too, and the docstring says
whether it would have passed the defect."""
import pytest
import torch

from distributed_lion_pytorch_amd.ops import fused
from lora_exact_cases import (BF16, DROPS, EMPTY_PARTS, MIN_TIE_SHARE, RANKS, ROWS_K, ROWS_K_SWEEP, ROWS_M, ROWS_M_SWEEP,
                              UP_M, UP_M_SWEEP, UP_N, UP_N_SWEEP, case_scale, cols_ref, dx_operands, keep_mask,
                              probe_decode, probe_weights, probe_windows, rows_operands, rows_ref, strided, up_operands,
                              up_ref)
from numerics import assert_bits, assert_part_sums, drop_consts, lora_parts, tie_share

UP_CASES = [(UP_M, n) for n in UP_N_SWEEP] + [(m, UP_N) for m in UP_M_SWEEP] + [EMPTY_PARTS]


def _old_rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-6))


def _rejected(got, ref, name):
    with pytest.raises(AssertionError, match="elements differ"):
        assert_bits(got, ref, name)


# --------------------------------------------------------------------------- generators
def test_drop_consts_are_exact_powers_of_two():
    assert drop_consts(0.0) == (0, 1.0) and drop_consts(0.5) == (32768, 2.0) and drop_consts(0.75) == (49152, 4.0)
    th, inv = drop_consts(0.1)
    assert th == 6554 and inv == float(torch.tensor(65536.0 / (65536 - 6554), dtype=torch.float32))


@pytest.mark.parametrize("r", RANKS)
def test_rows_cases_are_exact(r):
    for M, K in [(ROWS_M, k) for k in ROWS_K_SWEEP] + [(m, ROWS_K) for m in ROWS_M_SWEEP]:
        x, a = rows_operands(M, K, r)
        assert not torch.equal(a[0], a[1])  # swapped rows of a are another matrix
        for p in DROPS:
            u = rows_ref(x, a, case_scale(K, r), p, 7)  # asserts max sum |xd a| < 2^24
            assert u.shape == (M, r) and torch.isfinite(u.float()).all()
        if K > 4096:  # the columns of a second pass carry weight
            assert float((x[:, 4096:].float() @ a[:, 4096:].float().t()).abs().min(1)[0].max()) > 0


@pytest.mark.parametrize("M,N", UP_CASES)
@pytest.mark.parametrize("r", RANKS)
def test_up_cols_cases_are_exact_and_full_of_ties(r, M, N):
    s = case_scale(M, N, r)
    x, a = rows_operands(M, ROWS_K, r)
    o, b, dout = up_operands(M, N, r)
    xx, aa, dd, bb = dx_operands(M, N, r)
    for p in (0.5, 0.75):
        u = rows_ref(x, a, 1.0, p, 20231)
        out, inner, total = up_ref(o, u, b, s)  # asserts both sums exact in fp32
        ti, ts = tie_share(inner), tie_share(total)
        print(f"[ties] M={M} N={N} r={r} p={p}: adapter term {ti:.3f}, sum {ts:.3f}")
        assert ti >= MIN_TIE_SHARE and ts >= MIN_TIE_SHARE
        cols_ref(dout, u, None, s)
    du = rows_ref(dd, bb.t().contiguous(), s)
    assert bool((du > 0).all()) and bool((aa > 0).all())
    for p in (0.0, 0.5, 0.75):
        part, dx = cols_ref(xx, du, aa, 1.0, p, 3)
        assert torch.equal(dx != 0, keep_mask(M, N, p, 3))
        assert part.shape == (lora_parts(M, N)[0], r, N)


# --------------------------------------------------------------------------- part ranges
def test_part_ranges_follow_the_documented_rule():
    P, rpp, ranges = lora_parts(*EMPTY_PARTS)
    assert (P, rpp) == (512, 17)
    empty = [p for p, (r0, r1) in enumerate(ranges) if r1 <= r0]
    assert empty == list(range(483, 512)) and len(empty) == 29
    assert ranges[482] == (8194, 8200) and ranges[483] == (8200, 8200)
    assert lora_parts(67, 520)[:2] == (5, 14) and lora_parts(67, 512)[:2] == (5, 14)
    assert lora_parts(1027, 768)[:2] == (65, 16) and lora_parts(1, 32)[:2] == (1, 1)
    assert lora_parts(130, 4096)[:2] == (9, 15) and lora_parts(100000, 11008)[0] == 23
    for rows in (1, 5, 16, 17, 100, 1027, 8200):
        for N in (32, 480, 512, 520, 768, 11008):
            P, rpp, rg = lora_parts(rows, N)
            assert P == max(1, min(512 // ((N + 511) // 512), (rows + 15) // 16)) and len(rg) == P
            assert rg[0][0] == 0 and max(r1 for _, r1 in rg) == rows
            assert all(a[1] == b[0] for a, b in zip(rg, rg[1:])) and all(0 <= r1 - r0 <= rpp for r0, r1 in rg)


def test_assert_part_sums_checks_each_part_on_its_own_range():
    M, N, r = 100, 520, 8
    _, _, dout = up_operands(M, N, r)
    u = rows_ref(*rows_operands(M, ROWS_K, r), 1.0)
    _, _, ranges = lora_parts(M, N)
    good, _ = cols_ref(dout, u, None, 2.0)
    assert_part_sums(good, dout, u, ranges, "nr", 2.0, exact=True, name="good")
    moved = good.clone()  # one row's contribution moved to the neighbouring part: the total is unchanged
    delta = 2.0 * dout[ranges[1][0]].float()[:, None] * u[ranges[1][0]].float()[None, :]
    moved[1] -= delta
    moved[0] += delta
    assert torch.equal(moved.sum(0), good.sum(0))
    with pytest.raises(AssertionError, match="elements differ"):
        assert_part_sums(moved, dout, u, ranges, "nr", 2.0, exact=True, name="moved")
    with pytest.raises(AssertionError, match="over n"):
        assert_part_sums(moved, dout, u, ranges, "nr", 2.0, name="moved, bound")
    assert assert_part_sums(good, dout, u, ranges, "nr", 2.0, name="good, bound") == 0.0
    neg = torch.cat([good, -torch.zeros(1, N, r)])  # an empty part of -0
    with pytest.raises(AssertionError, match="without rows"):
        assert_part_sums(neg, dout, u, ranges + [(M, M)], "nr", 2.0, exact=True, name="-0")


# --------------------------------------------------------------------------- the mask probe
def _probe_ref(M, K, r, p, seed, defect=None, ld=None):
    ones = torch.ones(M, K, dtype=BF16)
    us = [rows_ref(ones, probe_weights(K, r, w), 2.0, p, seed, defect, ld) for w in range(probe_windows(K, r))]
    return probe_decode(us, K, r, 2.0, p)


@pytest.mark.parametrize("r", RANKS)
def test_probe_reads_every_keep_bit(r):
    for M, K, p in [(33, 256, 0.5), (17, 288, 0.75), (3, 4128, 0.5)]:
        host = fused.norm_dropout_keep(M, K, p, 20231)
        assert torch.equal(_probe_ref(M, K, r, p, 20231), host)
        # any single flipped bit is seen
        flipped = _probe_ref(M, K, r, p, 20231, "flip_bit")
        assert int((flipped != host).sum()) == 1
    assert bool(_probe_ref(5, 64, r, 0.0, 1).all())


# --------------------------------------------------------------------------- planted defects
@pytest.mark.parametrize("r", RANKS)
def test_defect_flipped_keep_bit(r):
    """One keep bit flipped in one element.  Old criterion (its own shape and randn data, M = 1027, K = 512,
    N = 768, p = 0.1): the flipped element moves its row of the output by 0.5 .. 3 % of the tensor's maximum
    depending on |x a| there -- on either side of the 1e-2 bound, so it is caught by luck only; dA (one product in
    a sum of M) passes; dx (one element of full size) is caught."""
    M, K, N, p = 1027, 512, 768, 0.5
    g = torch.Generator().manual_seed(0)
    xr, orr = torch.randn(M, K, generator=g).to(BF16), torch.randn(M, N, generator=g).to(BF16)
    ar, br = (torch.randn(r, K, generator=g) * 0.05).to(BF16), (torch.randn(N, r, generator=g) * 0.05).to(BF16)
    ug, ub = rows_ref(xr, ar, 1.0, 0.1, 5, exact=False), rows_ref(xr, ar, 1.0, 0.1, 5, "flip_bit", exact=False)  # its p
    assert not torch.equal(ug, ub)
    rel = _old_rel(up_ref(orr, ub, br, 2.0, exact=False)[0], up_ref(orr, ug, br, 2.0, exact=False)[0])
    print(f"flipped keep bit: old criterion on out {rel:.5f}")
    assert 1e-3 < rel < 5e-2
    x, a = rows_operands(33, 256, r)
    x = torch.where(x == 0, torch.ones((), dtype=BF16), x)  # the flipped element's value must matter
    _rejected(rows_ref(x, a, 2.0, p, 5, "flip_bit"), rows_ref(x, a, 2.0, p, 5), "u")
    assert int((_probe_ref(33, 256, r, p, 5, "flip_bit") != fused.norm_dropout_keep(33, 256, p, 5)).sum()) == 1
    xx, aa, dd, bb = dx_operands(M, K, r)
    du = rows_ref(dd, bb.t().contiguous(), 2.0)
    (gp, gdx), (bp, bdx) = cols_ref(xx, du, aa, 1.0, p, 5), cols_ref(xx, du, aa, 1.0, p, 5, "flip_bit")
    _rejected(bdx, gdx, "dx")
    assert int(((bdx != 0) != keep_mask(M, K, p, 5)).sum()) == 1
    assert _old_rel(bdx, gdx) > 2e-2  # dx itself: one element of the size of the maximum -- the old test sees this one
    assert _old_rel(bp.sum(0), gp.sum(0)) < 2e-2  # dA: it does not


@pytest.mark.parametrize("r", RANKS)
def test_defect_mask_indexed_with_row_stride(r):
    """Mask index t * ld + c instead of t * K + c on a strided operand.  Old criterion: never ran a strided x;
    on one it passes u (another valid mask, error ~ sqrt(K) products) only by chance and fails dx."""
    M, K, p = 33, 256, 0.5
    x, a = rows_operands(M, K, r)
    ld = strided(x).stride(0)
    assert ld == K + 24
    _rejected(rows_ref(x, a, 2.0, p, 5, "mask_stride", ld), rows_ref(x, a, 2.0, p, 5), "u")
    xx, aa, dd, bb = dx_operands(M, K, r)
    du = rows_ref(dd, bb.t().contiguous(), 2.0)
    (gp, gdx), (bp, bdx) = cols_ref(xx, du, aa, 1.0, p, 5), cols_ref(xx, du, aa, 1.0, p, 5, "mask_stride", ld)
    _rejected(bdx, gdx, "dx")
    _rejected(bp, gp, "dA partials")
    assert torch.equal(rows_ref(x, a, 2.0, 0.0, 5, "mask_stride", ld), rows_ref(x, a, 2.0, 0.0, 5))  # p = 0 cannot see it


@pytest.mark.parametrize("r", RANKS)
def test_defect_k_tail_dropped(r):
    """lora_rows' outer loop runs once.  Exactly the K > 4096 cases differ.  Old criterion: K = 512 only, never reached."""
    for K in ROWS_K_SWEEP:
        x, a = rows_operands(ROWS_M, K, r)
        good, bad = rows_ref(x, a, 1.0), rows_ref(x, a, 1.0, defect="k_tail")
        if K > 4096:
            _rejected(bad, good, f"K={K}")
            if K == 4128:
                print(f"K=4128 old criterion: {_old_rel(bad, good):.4f}")
        else:
            assert torch.equal(bad, good)


@pytest.mark.parametrize("r", RANKS)
def test_defect_partials_transposed(r):
    """[N][R] written as [R][N] and back.  Old criterion: rejects it too (the gradient is scrambled)."""
    M, N = 67, 520
    _, _, dout = up_operands(M, N, r)
    u = rows_ref(*rows_operands(M, ROWS_K, r), 1.0)
    good, bad = cols_ref(dout, u, None, 2.0)[0], cols_ref(dout, u, None, 2.0, defect="swap_layout")[0]
    assert good.shape == bad.shape
    _rejected(bad, good, "cols0")
    assert _old_rel(bad.sum(0), good.sum(0)) > 2e-2
    xx, aa, dd, bb = dx_operands(M, N, r)
    du = rows_ref(dd, bb.t().contiguous(), 2.0)
    _rejected(cols_ref(xx, du, aa, 1.0, 0.5, 5, "swap_layout")[0], cols_ref(xx, du, aa, 1.0, 0.5, 5)[0], "cols1")


@pytest.mark.parametrize("r", RANKS)
def test_defect_tail_batch_counted_twice(r):
    """The last batch of 4 rows of one part enters twice.  Old criterion: rejects it at its shape with randn data
    (0.06 .. 0.10 of the maximum: the sums of 1027 randn products cancel, 4 doubled rows do not), but it cannot
    say which part is wrong, and the margin shrinks like 1 / sqrt(M).  The per-part bound rejects it at any M."""
    M, N = 1027, 768
    _, _, dout = up_operands(M, N, r)
    u = rows_ref(*rows_operands(M, ROWS_K, r), 1.0)
    good, bad = cols_ref(dout, u, None, 2.0)[0], cols_ref(dout, u, None, 2.0, defect="tail_twice")[0]
    _rejected(bad, good, "cols0")
    assert torch.equal(bad[1:], good[1:])
    g = torch.Generator().manual_seed(0)
    dr, ur = torch.randn(M, N, generator=g).to(BF16), torch.randn(M, r, generator=g).to(BF16)
    good, bad = cols_ref(dr, ur, None, 2.0, exact=False)[0], cols_ref(dr, ur, None, 2.0, defect="tail_twice", exact=False)[0]
    rel = _old_rel(bad.sum(0), good.sum(0))
    print(f"tail counted twice, randn M={M}: old criterion {rel:.4f}")
    with pytest.raises(AssertionError, match="over n"):
        assert_part_sums(bad, dr, ur, lora_parts(M, N)[2], "nr", 2.0, name="tail twice")
    assert_part_sums(good, dr, ur, lora_parts(M, N)[2], "nr", 2.0, name="good")


@pytest.mark.parametrize("defect", ["no_inner_rounding", "half_up"])
@pytest.mark.parametrize("r", RANKS)
def test_defect_up_roundings(r, defect):
    """lora_up without the bf16 rounding of the adapter term, or with ties rounded away from zero.  Old criterion:
    passes both (one bf16 ulp, 2^-8 relative, in some elements)."""
    M, N, s = 67, 520, 2.0
    u = rows_ref(*rows_operands(M, ROWS_K, r), 1.0, 0.5, 20231)
    o, b, _ = up_operands(M, N, r)
    good, bad = up_ref(o, u, b, s)[0], up_ref(o, u, b, s, defect)[0]
    _rejected(bad, good, defect)
    share = float((bad != good).double().mean())
    print(f"{defect}: {share:.3f} of the elements differ, old criterion {_old_rel(bad, good):.5f}")
    assert share >= 0.01 and _old_rel(bad, good) < 1e-2
    if defect == "half_up":  # ... and of the rows kernel's and dx's rounding
        x, a = rows_operands(ROWS_M, 4096, r)
        _rejected(rows_ref(x, a, 1.0, defect=defect), rows_ref(x, a, 1.0), "u half up")
