"""Hand-built inputs for the 4-bit kernels (csrc/quant.hip), shared by
test_quant_gpu.py and test_quant_cpu.py: blocks that meet the tie rule, the
sign of zero and the tail guards of quant4, and packed bytes / absmax values
that drive the expansion to the ends of the fp16 range."""
import torch

from distributed_lion_pytorch_amd.ops.quant import code_tensor

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
QUANT_BLOCKS = [1, 255, 256, 257]  # around the 256 blocks a thread block of quant4 takes
# words (8 elements) of dequant4_: a thread block takes 4 steps of 256 words.  The first three are n = 64,
# 64 * 129 and 8 * (1024 * 3 + 5) rounded up to a block; the last two leave 2 and 3 live steps in the last block
DEQUANT_WORDS = [8, 1032, 3080, 1024 + 256 + 8, 2048 + 512 + 8]
DEQUANT_T_SHAPES = [(64, 128), (64, 384), (192, 128), (128, 256)]  # (N, K): one tile, a row / column of tiles, 2 x 2

# absmax values of the hand-built expansion input
EDGE_ABSMAX = [2.0 ** e for e in range(-30, 18)] + [0.005, 65504.0, 65519.0, 65520.0, 3.0e38]


def tie_points(qt):
    """fp32 x that lie exactly midway between two codebook entries which are both the nearest ones
    (|x - a| == |x - b| == min over the codebook, all in fp32): where ``<`` and ``<=`` pick different indices."""
    code = code_tensor(qt)
    vals = torch.unique(code)  # sorted; FP4's +0 and -0 are one value
    out = []
    for a, b in zip(vals[:-1].tolist(), vals[1:].tolist()):
        x = (torch.tensor(a, dtype=torch.float32) + torch.tensor(b, dtype=torch.float32)) / 2
        d = (x - code).abs()
        da, db = (x - torch.tensor(a)).abs(), (x - torch.tensor(b)).abs()
        if da == db and da == d.min():
            out.append(float(x))
    return out


def crafted_blocks(qt, dt):
    """[9, 64] of dtype dt.  Block 0: absmax 1 with the codebook's tie points (those exact in dt stay ties), the
    codes themselves and +-0.75, +-0.5; 1: +0 / -0 beside one 2.0; 2: the maximum is negative; 3, 4: one repeated
    value (positive, negative); 5: all zero; 6: the largest finite values of dt; 7: subnormals of dt (fp32:
    small normals); 8: a single non-zero element."""
    ties = tie_points(qt)
    v0 = [1.0] + [s * t for t in ties for s in (1.0, -1.0)] + [0.75, -0.75, 0.5, -0.5, 0.375, -0.375, 0.0, -0.0]
    v0 += code_tensor(qt).tolist()
    b0 = torch.tensor((v0 * 64)[:64], dtype=torch.float32)
    b1 = torch.tensor([0.0, -0.0] * 32, dtype=torch.float32)
    b1[17] = 2.0
    b2 = torch.linspace(0.0, 0.9, 64)
    b2[40] = -3.0
    b3, b4 = torch.full((64,), 0.7), torch.full((64,), -0.3)
    b5 = torch.zeros(64)
    big = {torch.bfloat16: 3.0e38, torch.float16: 65504.0, torch.float32: 3.0e38}[dt]
    b6 = torch.tensor(big, dtype=torch.float32) * torch.linspace(-1.0, 1.0, 64)
    tiny = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24, torch.float32: 2.0 ** -100}[dt]
    b7 = torch.arange(-31, 33, dtype=torch.float64) * tiny
    b8 = torch.zeros(64)
    b8[63] = -1.5
    w = torch.stack([b.double() for b in (b0, b1, b2, b3, b4, b5, b6, b7, b8)]).to(dt)
    assert torch.isfinite(w.float()).all()
    return w


def edge_packed():
    """(q uint8 [n / 2], absmax fp32 [n / 64]): every byte value 0 .. 255 under every absmax of EDGE_ABSMAX
    (8 blocks of 32 bytes each)."""
    q = torch.arange(256, dtype=torch.uint8).repeat(len(EDGE_ABSMAX))
    absmax = torch.tensor(EDGE_ABSMAX, dtype=torch.float32).repeat_interleave(8)
    assert q.numel() * 2 == absmax.numel() * 64
    return q, absmax


def random_packed(nblocks, seed):
    """Random bytes and absmax values drawn from EDGE_ABSMAX's middle (2^-12 .. 2^4: finite in every dtype)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 256, (nblocks * 32,), generator=g, dtype=torch.uint8)
    e = torch.randint(-12, 5, (nblocks,), generator=g)
    absmax = torch.ldexp(torch.ones(nblocks), e) * (1 + torch.rand(nblocks, generator=g))
    return q, absmax.float()
