"""test_lora_wide_exact_gpu.py's cases without a GPU: every parametrised case
meets the exactness and tie-share conditions of the closed forms at r in {32,
64, 128}, the part ranges follow the documented wide rule, two defects of a
tiled rank dimension planted in the closed forms are rejected by the bit
comparison the GPU tests apply, and no LoRA kernel -- wide or narrow -- uses
scratch memory (hipcc cross-compiles)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from distributed_lion_pytorch_amd.ops import fused
from lora_exact_cases import (DROPS, MIN_TIE_SHARE, ROWS_K, ROWS_M, ROWS_M_SWEEP, UP_M, UP_M_SWEEP, UP_N, case_scale,
                              dx_operands, keep_mask, rows_operands, rows_ref, up_operands, up_ref)
from lora_wide_cases import (EMPTY_PARTS, ROWS_K_SWEEP, UP_N_SWEEP, WIDE_RANKS, cols_ref_wide, drop_tiles, swap_tiles,
                             wide_parts)
from numerics import assert_bits, lora_parts, tie_share

UP_CASES = [(UP_M, n) for n in UP_N_SWEEP] + [(m, UP_N) for m in UP_M_SWEEP]


def _rejected(got, ref, name):
    with pytest.raises(AssertionError, match="elements differ"):
        assert_bits(got, ref, name)


# --------------------------------------------------------------------------- generators
@pytest.mark.parametrize("r", WIDE_RANKS)
def test_rows_cases_are_exact(r):
    for M, K in [(ROWS_M, k) for k in ROWS_K_SWEEP] + [(m, ROWS_K) for m in ROWS_M_SWEEP]:
        x, a = rows_operands(M, K, r)
        assert not torch.equal(a[0], a[16])  # swapped tiles of a are another matrix
        for p in DROPS:
            u = rows_ref(x, a, case_scale(K, r), p, 7)  # asserts max sum |xd a| < 2^24
            assert u.shape == (M, r) and torch.isfinite(u.float()).all()


@pytest.mark.parametrize("M,N", UP_CASES + [EMPTY_PARTS])
@pytest.mark.parametrize("r", WIDE_RANKS)
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
        if p == 0.5:  # the u the GPU file feeds lora_up (its default p); at 0.75 only the exactness is needed
            assert ti >= MIN_TIE_SHARE and ts >= MIN_TIE_SHARE
        cols_ref_wide(dout, u, None, s)
    du = rows_ref(dd, bb.t().contiguous(), s)
    assert bool((du > 0).all()) and bool((aa > 0).all())
    for p in (0.0, 0.5, 0.75):
        part, dx = cols_ref_wide(xx, du, aa, 1.0, p, 3)
        assert torch.equal(dx != 0, keep_mask(M, N, p, 3))
        assert part.shape == (wide_parts(M, N, r)[0], r, N)


# --------------------------------------------------------------------------- part ranges
def test_wide_part_ranges_follow_the_documented_rule():
    P, rpp, ranges = wide_parts(*EMPTY_PARTS, 32)
    assert (P, rpp) == (200, 65)
    assert [p for p, (r0, r1) in enumerate(ranges) if r1 <= r0] == [197, 198, 199]
    assert ranges[196] == (12740, 12801) and ranges[197] == (12801, 12801)
    assert wide_parts(*EMPTY_PARTS, 64)[:2] == (100, 129) and wide_parts(*EMPTY_PARTS, 128)[:2] == (50, 257)
    assert wide_parts(4096, 4096, 128)[:2] == (16, 256) and wide_parts(4096, 4096, 32)[:2] == (32, 128)
    assert wide_parts(1027, 768, 32)[:2] == (16, 65) and wide_parts(67, 520, 64)[:2] == (1, 67)
    for r in WIDE_RANKS:
        for rows in (1, 5, 16, 17, 100, 1027, 4096, 12801):
            for N in (32, 128, 136, 520, 768, 4096, 11008):
                P, rpp, rg = wide_parts(rows, N, r)
                cblocks = (N + 127) // 128
                assert P == max(1, min(-(-1024 // cblocks), rows // (2 * r))) and len(rg) == P
                # the fp32 partials never exceed the bytes of the bf16 g operand, one part aside
                assert P == 1 or P * N * r * 4 <= rows * N * 2
                assert rg[0][0] == 0 and max(r1 for _, r1 in rg) == rows
                assert all(a[1] == b[0] for a, b in zip(rg, rg[1:])) and all(0 <= r1 - r0 <= rpp for r0, r1 in rg)
    # the narrow ranks keep their rule (numerics.lora_parts)
    for r in (8, 16):
        for rows, N in ((67, 520), (1027, 768), (8200, 32), (100000, 11008)):
            assert fused.lora_cols_parts(rows, N, r) == lora_parts(rows, N)
    # 4096 tokens, N = 4096, r = 128: the narrow rule's 64 parts would be 128 MiB of partials beside 32 MiB of g
    assert lora_parts(4096, 4096)[0] * 4096 * 128 * 4 == 4 * (4096 * 4096 * 2)
    assert wide_parts(4096, 4096, 128)[0] * 4096 * 128 * 4 == 4096 * 4096 * 2


# --------------------------------------------------------------------------- planted defects
@pytest.mark.parametrize("defect", [drop_tiles, swap_tiles], ids=["tiles_dropped", "tiles_swapped"])
@pytest.mark.parametrize("r", WIDE_RANKS)
def test_defect_in_the_rank_tiles(r, defect):
    """A kernel that runs only the first 16-wide rank tile, or that exchanges two of them, in each of the three
    ops: the rank is the output dimension of lora_rows and of both partial layouts, and the contraction of lora_up
    and dx (there the tiles of one operand move against the other's)."""
    M, N, p, s = UP_M, UP_N, 0.5, 2.0
    x, a = rows_operands(M, ROWS_K, r)
    u = rows_ref(x, a, 1.0, p, 5)
    _rejected(defect(u, 1), u, "u")
    _rejected(rows_ref(x, defect(a, 0), 1.0, p, 5), u, "u from a")
    o, b, dout = up_operands(M, N, r)
    _rejected(up_ref(o, defect(u, 1), b, s)[0], up_ref(o, u, b, s)[0], "out")
    part0 = cols_ref_wide(dout, u, None, s)[0]
    _rejected(defect(part0, 2), part0, "cols0")
    xx, aa, dd, bb = dx_operands(M, N, r)
    du = rows_ref(dd, bb.t().contiguous(), s)
    part1, dx = cols_ref_wide(xx, du, aa, 1.0, p, 5)
    _rejected(defect(part1, 1), part1, "cols1")
    _rejected(cols_ref_wide(xx, defect(du, 1), aa, 1.0, p, 5)[1], dx, "dx")


# --------------------------------------------------------------------------- spill guard
CSRC = Path(__file__).resolve().parent.parent / "distributed_lion_pytorch_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _lora_kernel_resources(src, tmp_path):
    from distributed_lion_pytorch_amd._build import EXTRA_FLAGS

    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", f"-I{CSRC}", *EXTRA_FLAGS.get(src, []), "-c",
           str(CSRC / src), "-o", str(tmp_path / (src + ".o")), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark: *(VGPRs Spill|SGPRs Spill|VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return {k: v for k, v in out.items() if re.search(r"lora_\w+_kernel", k)}


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
@pytest.mark.parametrize("src,count", [("lora.hip", 10), ("lora_wide.hip", 15)])
def test_lora_kernels_use_no_scratch(src, count, tmp_path):
    """Every instantiation of the LoRA kernels -- rows with and without dropout, up, cols in both modes, at each
    rank -- compiles without scratch: none in the wide kernels, and none appears in the narrow ones."""
    res = _lora_kernel_resources(src, tmp_path)
    assert len(res) == count, sorted(res)
    for name, v in res.items():
        print(f"{name}: {v}")
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
