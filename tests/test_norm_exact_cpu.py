"""CPU companion of test_norm_exact_gpu.py: the generators, closed forms and
exactness preconditions of norm_exact_cases.py, and proof that the case lists
bite -- the fp32 emulations of add_norm_fwd / add_norm_bwd pass every case the
GPU file runs, and each planted defect (1 / capacity for 1 / C, the variance
taken over the padding as well, a row group missing from the backward's fold,
truncation for round-to-nearest-even) is rejected by them."""
import functools

import pytest
import torch

import norm_exact_cases as nc
from numerics import tie_share


def _fwd(defect=None):
    return functools.partial(nc.emul_fwd, defect=defect)


def _bwd(defect=None):
    return functools.partial(nc.emul_bwd, defect=defect)


def test_capacity_and_block_rows():
    assert [nc.capacity(C) for C in nc.EXACT_WIDTHS] == nc.EXACT_WIDTHS
    assert [nc.capacity(C) for C in nc.TAIL_WIDTHS] == [512, 768, 1024, 2048, 4096, 7168, 8192]
    assert [nc.rows_per_block(C) for C in (1016, 1024, 1032)] == [4, 4, 1]
    # 37 rows, 4 per block iteration, 3 blocks: block 0 ends on the lone row 36 (one of its 4 row groups)
    sets = nc.block_rows(37, 768, 3)
    assert sets[0].tolist() == [0, 1, 2, 3, 12, 13, 14, 15, 24, 25, 26, 27, 36]
    assert sets[1].tolist() == [4, 5, 6, 7, 16, 17, 18, 19, 28, 29, 30, 31]
    for C in (768, 2048):
        for parts in nc.bwd_parts(37, C):
            sets = nc.block_rows(37, C, parts)
            assert sorted(torch.cat(sets).tolist()) == list(range(37))
        assert any(s.numel() == 0 for s in nc.block_rows(37, C, nc.bwd_parts(37, C)[-1]))
    assert nc.block_rows(37, 2048, 3)[2].tolist() == list(range(2, 37, 3))


def test_means_are_exact_in_fp32():
    """float32(m C) * float32(1 / C) == m for every mean and width used (and for the backward's a and b); m = 3
    is not usable: it fails at 896, 3584 and 7168."""
    for C in nc.WIDTHS:
        assert all(nc.mean_is_exact(m, C) for m in nc.MEANS), C
        assert nc.bwd_means_exact(C), C
    assert [C for C in (896, 3584, 7168) if not nc.mean_is_exact(3, C)] == [896, 3584, 7168]


@pytest.mark.parametrize("C", [264, 1024, 7168])
def test_generators(C):
    for p, has_y, has_bias in nc.FWD_CONFIGS[1:]:
        x, y, bias = nc.residual_case(C, 37, p, has_y, has_bias)
        _, v32, keep = nc.residual_expected(x, y, bias, p, 4242)
        assert float(v32.abs().max()) <= 495 and bool((v32 == v32.round()).all())
        assert tie_share(v32.double()) >= nc.MIN_TIE_SHARE
        assert abs(float(keep.float().mean()) - (1 - p)) < 0.02
    x, y, bias, xo, m, d = nc.stats_case(C, 37, 0.75, True, True)
    assert bool((d.sum(-1) == 0).all()) and float(d.abs().max()) <= 16 and float(x.float().abs().max()) <= 256
    assert torch.equal(xo.float().sum(-1), m * C)
    c = nc.bwd_case(C, 37, False, True)
    assert torch.equal(((c["xo"].float() - c["mean"][:, None]) * c["rstd"][:, None]), c["s"])
    assert torch.equal(c["gd"].sum(-1), c["a"] * C) and torch.equal((c["gd"] * c["s"]).sum(-1), c["b"] * C)
    assert tie_share(c["t"].double()) >= nc.MIN_TIE_SHARE
    # the column pattern of w differs between any two 4-column chunks a lane could confuse
    w = c["gd"] - c["a"][:, None] - c["b"][:, None] * c["s"]
    assert len({tuple(w[:, i:i + 4].flatten().tolist()) for i in range(0, C // 2, 4)}) == C // 8


@pytest.mark.parametrize("C,rms", nc.CASES)
def test_emulation_passes_every_case(C, rms):
    for rows in nc.ROWS:
        assert nc.run_fwd_residual(_fwd(), C, rms, rows, "cpu") >= nc.MIN_TIE_SHARE
    assert nc.run_fwd_stats(_fwd(), C, rms, "cpu") <= 1.0
    nc.run_fwd_offset(_fwd(), C, rms, "cpu")
    assert nc.run_bwd_exact(_bwd(), C, rms, "cpu") >= nc.MIN_TIE_SHARE
    nc.run_bwd_randn(_bwd(), C, rms, "cpu")


def _rejected(fn, *args):
    try:
        fn(*args)
    except AssertionError as e:
        return str(e).splitlines()[0]
    return None


# tail widths whose capacity is wider than the row (7168 fills its capacity: nothing to get wrong there)
PADDED = [C for C in nc.TAIL_WIDTHS if nc.capacity(C) != C]


@pytest.mark.parametrize("C", PADDED)
def test_defect_inv_cap(C):
    """1 / capacity instead of 1 / C moves rstd by 0.4 % at 1016 and 0.05 % at 8184: the exact statistics (both
    norms), the mean bits of the residual cases and the offset rows all reject it."""
    assert "rstd" in _rejected(nc.run_fwd_stats, _fwd("inv_cap"), C, True, "cpu")
    for rms in (False, True):
        assert _rejected(nc.run_fwd_offset, _fwd("inv_cap"), C, rms, "cpu")
    assert "mean" in _rejected(nc.run_fwd_residual, _fwd("inv_cap"), C, False, 5, "cpu")
    assert "mean" in _rejected(nc.run_fwd_stats, _fwd("inv_cap"), C, False, "cpu")


@pytest.mark.parametrize("C", PADDED)
def test_defect_unmasked_variance(C):
    """The padding adding (0 - mean)^2 to the variance: rejected by the rows with a non-zero mean (LayerNorm; an
    RMSNorm has no mean to subtract)."""
    assert "rstd" in _rejected(nc.run_fwd_stats, _fwd("unmasked_var"), C, False, "cpu")
    assert "rstd" in _rejected(nc.run_fwd_offset, _fwd("unmasked_var"), C, False, "cpu")
    assert _rejected(nc.run_fwd_stats, _fwd("unmasked_var"), C, True, "cpu") is None


@pytest.mark.parametrize("C", [C for C in nc.WIDTHS if C <= 1024])
def test_defect_dropped_fold_group(C):
    for rms in (False, True):
        assert "dgamma" in _rejected(nc.run_bwd_exact, _bwd("drop_fold_group"), C, rms, "cpu")


@pytest.mark.parametrize("C", [256, 1032])
def test_defect_truncation(C):
    assert " h:" in _rejected(nc.run_fwd_residual, _fwd("trunc"), C, False, 5, "cpu")
    assert " xo:" in _rejected(nc.check_fwd_residual, _fwd("trunc"), C, False, 5, nc.FWD_CONFIGS[3], "pow2", "cpu")
    assert _rejected(nc.run_fwd_stats, _fwd("trunc"), C, True, "cpu")
    assert "dx" in _rejected(nc.run_bwd_exact, _bwd("trunc"), C, False, "cpu")
    assert _rejected(nc.run_bwd_randn, _bwd("trunc"), C, True, "cpu")
