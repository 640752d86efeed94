"""Pure-PyTorch oracle of the Distributed Lion semantics.

This module restates the behavioural contract of the reference optimizer
(``/root/reference/distributed_lion.py``) with plain ATen ops
so that it can serve three purposes:

1. the numerics oracle that the gfx950 kernels are tested against (bf16
   results are bit-identical because both round after every ATen-visible op);
2. the CPU execution path (gloo multi-process tests, no GPU);
3. the reference-compatible *functional* API (``update_fn``,
   ``update_fn_distributed``, ``update_fn_distributed_stoc``, ``majority_vote``,
   ``flatten_and_pad``, ``restore_flattened_tensor``), including an optional
   ``wire_dtype=torch.int64`` that reproduces the reference's 1 byte/param
   payload for A/B benchmarking.

Known reference defects are fixed here, explicitly: the stochastic path stores
and uses ``max_grad_norm`` (D2), does a real update at W == 1 (D3) and clamps
the Bernoulli probability (D4).
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.distributed as dist

# tie rules for an even split of votes
TIE_NEGATIVE = 0  # reference parity: torch.mode over {False, True} ties -> False -> delta = -1
TIE_ZERO = 1
TIE_POSITIVE = 2
TIE_CODES = {"negative": TIE_NEGATIVE, "ref_negative": TIE_NEGATIVE, "zero": TIE_ZERO, "positive": TIE_POSITIVE}

VOTE_MAJORITY = 0
VOTE_AVERAGE = 1
VOTE_PREVOTED = 2
VOTE_COUNTED = 3  # average from the gathered count bit planes (a2a path)
VOTE_CODES = {"majority": VOTE_MAJORITY, "average": VOTE_AVERAGE}


def exists(val) -> bool:
    return val is not None


# ------------------------------------------------------------------ codec
def flatten_and_pad(tensor: torch.Tensor, multiple: int = 8):
    """Flatten and zero-pad to a multiple of ``multiple`` (ref :14-24)."""
    flat = tensor.reshape(-1)
    pad = (-flat.numel()) % multiple
    if pad:
        flat = torch.cat([flat, flat.new_zeros(pad)])
    return flat, tensor.shape


def restore_flattened_tensor(padded: torch.Tensor, original_shape) -> torch.Tensor:
    """Drop padding and reshape (ref :27-31)."""
    n = 1
    for s in original_shape:
        n *= int(s)
    return padded[:n].reshape(original_shape)


_SHIFTS = {}


def _shifts(device) -> torch.Tensor:
    key = str(device)
    if key not in _SHIFTS:
        _SHIFTS[key] = torch.arange(8, dtype=torch.uint8, device=device)
    return _SHIFTS[key]


def pack_bits(bits: torch.Tensor, nbits: Optional[int] = None) -> torch.Tensor:
    """bool[n] -> uint8[ceil(nbits/8)], little-endian inside each byte.

    Element ``e`` lands in byte ``e // 8``, bit ``e % 8`` -- the reference's
    layout (ref :75-77) at 1 bit per element.
    """
    flat = bits.reshape(-1).to(torch.uint8)
    nbits = flat.numel() if nbits is None else nbits
    pad = nbits - flat.numel()
    if pad < 0:
        raise ValueError("nbits smaller than the bit count")
    pad += (-nbits) % 8
    if pad:
        flat = torch.cat([flat, flat.new_zeros(pad)])
    return (flat.view(-1, 8) << _shifts(flat.device)).sum(dim=1, dtype=torch.uint8)


def unpack_bits(packed: torch.Tensor, n: Optional[int] = None) -> torch.Tensor:
    """uint8[..., nb] -> bool[..., nb*8] (or the first ``n`` bits)."""
    out = ((packed.unsqueeze(-1) >> _shifts(packed.device)) & 1).bool()
    out = out.reshape(*packed.shape[:-1], packed.shape[-1] * 8)
    return out if n is None else out[..., :n]


def majority_vote(boolean_tensors: Sequence[torch.Tensor], tie: int = TIE_NEGATIVE) -> torch.Tensor:
    """Element-wise majority of W boolean tensors (ref :33-43).

    With the default tie rule an even split returns False, like ``torch.mode``
    in the reference.  Implemented with a popcount instead of ``stack + mode``.
    """
    count = torch.zeros(boolean_tensors[0].shape, dtype=torch.int32, device=boolean_tensors[0].device)
    for b in boolean_tensors:
        count += b.to(torch.int32)
    w = len(boolean_tensors)
    if tie == TIE_POSITIVE:
        return 2 * count >= w
    return 2 * count > w


# ------------------------------------------------------------ elementwise
def interp(grad: torch.Tensor, exp_avg: torch.Tensor, beta1: float) -> torch.Tensor:
    """beta1*m + (1-beta1)*g, rounded in the parameter dtype like the reference."""
    return exp_avg.clone().mul_(beta1).add_(grad, alpha=1 - beta1)


def sign_bits(grad: torch.Tensor, exp_avg: torch.Tensor, beta1: float) -> torch.Tensor:
    """Vote bit = sign(interp) > 0; zero and NaN vote negative (ref :68-71)."""
    return interp(grad, exp_avg, beta1) > 0


def stochastic_bits(grad, exp_avg, beta1: float, max_grad_norm: float, generator=None) -> torch.Tensor:
    """Stochastic binarization (ref :106-108), probability clamped to [0, 1] (D4)."""
    r = (1 + 1 / beta1) * max_grad_norm
    raw = interp(grad, exp_avg, beta1).float()
    prob = ((raw + r) / (2 * r)).clamp_(0.0, 1.0)
    return torch.bernoulli(prob, generator=generator) > 0


def momentum_update_(grad, exp_avg, beta2: float) -> None:
    exp_avg.mul_(beta2).add_(grad, alpha=1 - beta2)


def vote_delta(planes_bits: torch.Tensor, alive: torch.Tensor, mode: int = VOTE_MAJORITY,
               tie: int = TIE_NEGATIVE) -> torch.Tensor:
    """planes_bits: bool[W, n]; alive: bool/uint8[W]  ->  float32 delta[n].

    Matches lion_vote_apply_kernel: majority -> {+1, -1, tie}, average ->
    (2c - n_live) * (1/n_live), no voters -> 0.
    """
    alive_b = alive.to(torch.bool)
    n_live = int(alive_b.sum())
    if n_live == 0:
        return torch.zeros(planes_bits.shape[1], dtype=torch.float32, device=planes_bits.device)
    cnt = planes_bits[alive_b].to(torch.int32).sum(0)
    twice = 2 * cnt
    if mode == VOTE_AVERAGE:
        return _average_delta(cnt, n_live)
    tie_val = {TIE_NEGATIVE: -1.0, TIE_ZERO: 0.0, TIE_POSITIVE: 1.0}[tie]
    d = torch.full(cnt.shape, tie_val, dtype=torch.float32, device=cnt.device)
    d[twice > n_live] = 1.0
    d[twice < n_live] = -1.0
    return d


def _average_delta(cnt: torch.Tensor, n_live: int) -> torch.Tensor:
    """(2c - n_live) * fp32(1 / n_live): the kernels' expression for the average."""
    inv = torch.tensor(1.0 / n_live, dtype=torch.float32).item()
    return (2 * cnt - n_live).to(torch.float32) * inv


def count_plane_bits(world: int) -> int:
    """P: bit planes that hold a live-voter count of up to ``world``."""
    return int(world).bit_length()


def count_planes(planes_bits: torch.Tensor, alive: torch.Tensor, world: int) -> torch.Tensor:
    """bool[W, n] -> bool[P, n]: plane j is bit j of each coordinate's count of
    live voters (the K4c oracle), P = ``world.bit_length()``."""
    alive_b = alive.to(torch.bool)
    cnt = planes_bits[alive_b].to(torch.int32).sum(0)
    shifts = torch.arange(count_plane_bits(world), dtype=torch.int32, device=cnt.device)
    return ((cnt.unsqueeze(0) >> shifts.unsqueeze(1)) & 1).bool()


def counted_delta(count_bits: torch.Tensor, n_live: int) -> torch.Tensor:
    """bool[P, n] count planes -> float32 delta[n] of the average vote; the
    same expression as ``vote_delta``'s average branch, no voters -> 0."""
    if n_live == 0:
        return torch.zeros(count_bits.shape[1], dtype=torch.float32, device=count_bits.device)
    shifts = torch.arange(count_bits.shape[0], dtype=torch.int32, device=count_bits.device)
    cnt = (count_bits.to(torch.int32) << shifts.unsqueeze(1)).sum(0).to(torch.int32)
    return _average_delta(cnt, n_live)


def prevoted_delta(pos_bits: torch.Tensor, neg_bits: Optional[torch.Tensor]) -> torch.Tensor:
    neg = ~pos_bits if neg_bits is None else neg_bits
    d = torch.zeros(pos_bits.shape, dtype=torch.float32, device=pos_bits.device)
    d[neg] = -1.0
    d[pos_bits] = 1.0
    return d


def vote_reduce_bits(planes_bits: torch.Tensor, alive: torch.Tensor, tie: int):
    """bool[W, n] -> (pos bool[n], neg bool[n]) -- the K4 oracle."""
    alive_b = alive.to(torch.bool)
    n_live = int(alive_b.sum())
    if n_live == 0:
        z = torch.zeros(planes_bits.shape[1], dtype=torch.bool, device=planes_bits.device)
        return z, z.clone()
    twice = 2 * planes_bits[alive_b].to(torch.int32).sum(0)
    pos = (twice > n_live) | ((twice == n_live) & (tie == TIE_POSITIVE))
    neg = (twice < n_live) | ((twice == n_live) & (tie == TIE_NEGATIVE))
    return pos, neg


# ------------------------------------------------- stochastic rounding
# Opt-in rounding of the bf16 parameter store (Lion(param_rounding="stochastic")).
# Round-to-nearest drops every update below half a bf16 ulp: at lr 1e-4 no
# weight with |p| >= 2^-5 moves, and a decay of 1 - 1e-5 never does.  The
# stochastic store picks one of the two bf16 neighbours of the fp32 result
# with probability proportional to the remainder, so E[stored] == the fp32
# value.  The 16 random bits of a coordinate are a pure integer hash of
# (seed, step, global coordinate) -- the same on every rank, reproduced here
# with int64 arithmetic masked to 32 bits (csrc/common.h: sr_bf16, sr_hash).
ROUND_NEAREST = 0
ROUND_STOCHASTIC = 1
ROUNDING_CODES = {"nearest": ROUND_NEAREST, "stochastic": ROUND_STOCHASTIC}

_M32 = 0xFFFFFFFF


def _mix32(x):
    """The lowbias32 finaliser on a Python int or an int64 tensor of 32-bit values."""
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32
    return x ^ (x >> 16)


def sr_key(seed: int, step: int) -> int:
    """The 32-bit launch key that folds (seed, step): one per optimizer step,
    computed on the host, identical on every rank (no rank term)."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    k = _mix32((seed & _M32) ^ 0x9E3779B9)
    k = _mix32(k ^ (seed >> 32))
    k = _mix32((k + (step & _M32)) & _M32)
    return _mix32(k ^ (step >> 32))


def sr_bits16(coords: torch.Tensor, seed: int, step: int) -> torch.Tensor:
    """int64 r in [0, 65536) for each global coordinate (int64 tensor).  One
    32-bit hash per coordinate pair ``c >> 1``: mix32(mix32(lo32(pair) ^ key)
    + hi32(pair) * 0x9E3779B1 + 0x85EBCA6B); the low half belongs to the even
    coordinate, the high half to the odd one."""
    c = coords.to(torch.int64)
    pair = c >> 1
    h = _mix32((pair & _M32) ^ sr_key(seed, step))
    h = _mix32((h + ((pair >> 32) & _M32) * 0x9E3779B1 + 0x85EBCA6B) & _M32)
    return (h >> ((c & 1) * 16)) & 0xFFFF


def sr_bf16(x: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """fp32 ``x``, int64 ``r`` in [0, 65536) -> the bfloat16 whose bit pattern
    is ``(bits(x) + r) >> 16``: it rounds away from zero with probability
    low16(bits(x)) / 65536 over uniform r (unbiased for both signs), a
    representable x is unchanged for every r, the carry runs into the exponent
    (the largest finite value may become Inf); NaN and Inf round to nearest."""
    assert x.dtype == torch.float32
    bits = x.contiguous().view(torch.int32).to(torch.int64) & _M32
    out = (bits + r.to(torch.int64).view(x.shape)) & 0xFFFF0000
    out = torch.where(out >= 1 << 31, out - (1 << 32), out).to(torch.int32).view(torch.float32)
    return torch.where(torch.isfinite(x), out, x).to(torch.bfloat16)


def _fma32(a: float, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fp32 fma(a, b, c), correctly rounded, for fp32 tensors b and c and a
    scalar a (rounded to fp32): the product is exact in fp64; the fp64 sum is
    turned into its round-to-odd value (TwoSum error -> sticky bit), after
    which the rounding to fp32 cannot double-round."""
    a64 = torch.tensor(a, dtype=torch.float32, device=b.device).double()
    prod, c64 = a64 * b.double(), c.double()
    s = prod + c64
    t = s - prod
    err = (prod - (s - t)) + (c64 - t)
    sb = s.view(torch.int64)
    inexact = (err != 0) & torch.isfinite(s)
    toward_zero = inexact & ((err > 0) != (s > 0))  # |exact| < |s|: truncate by one ulp first
    odd = (sb - toward_zero.to(torch.int64)) | 1
    return torch.where(inexact, odd, sb).view(torch.float64).float()


def sr_bf16_(p: torch.Tensor, x: torch.Tensor, coords: torch.Tensor, seed: int, step: int) -> None:
    """Store fp32 ``x`` into the bf16 parameter ``p`` with the stochastic
    rounding of its coordinates under (seed, step)."""
    p.copy_(sr_bf16(x.reshape(-1), sr_bits16(coords, seed, step)).view(p.shape))


def _apply_stochastic_(p, delta, lr, wd, coords, seed, step) -> None:
    # ONE rounding: x = fma(-lr, delta, p * decay) with the decayed parameter
    # kept as an fp32 product -- on purpose not the nearest path's two bf16
    # roundings, so that both the decay and the step survive in expectation
    decay = torch.tensor(1 - lr * wd, dtype=torch.float32, device=p.device)
    x = _fma32(-lr, delta.reshape(-1).float(), p.reshape(-1).float() * decay)
    sr_bf16_(p, x, coords, seed, step)


def _stochastic(p: torch.Tensor, rounding: int) -> bool:
    if rounding not in (ROUND_NEAREST, ROUND_STOCHASTIC):
        raise ValueError(f"rounding must be one of {tuple(ROUNDING_CODES.values())}")
    if rounding == ROUND_STOCHASTIC and p.dtype == torch.float16:
        raise ValueError("stochastic parameter rounding supports bfloat16 (and is a no-op for float32), not float16")
    return rounding == ROUND_STOCHASTIC and p.dtype == torch.bfloat16  # an fp32 store is exact: nearest


def apply_delta_(p: torch.Tensor, delta: torch.Tensor, lr: float, wd: float, rounding: int = ROUND_NEAREST,
                 coords: Optional[torch.Tensor] = None, seed: int = 0, step: int = 0) -> None:
    """p <- round(round(p*(1-lr*wd)) - lr*delta)  (ref :64 then :92).

    ``rounding=ROUND_STOCHASTIC`` (bf16 p): p <- sr_bf16(fma(-lr, delta,
    p*(1-lr*wd))) with the bits of ``coords`` (the elements' global
    coordinates, int64) under ``(seed, step)``."""
    if _stochastic(p, rounding):
        return _apply_stochastic_(p, delta, lr, wd, coords, seed, step)
    p.mul_(1 - lr * wd)
    p.add_(delta.view(p.shape), alpha=-lr)


# ------------------------------------------- stochastic binarisation, exact
# The oracle of K3 (csrc/lion_kernels.hip: lion_encode_kernel<DT, true>): the
# kernel's Philox4x32-10 draw and its fp32 probability, reproduced with int64
# tensors masked to 32 bits and correctly rounded fp32 ops -- no
# torch.Generator, so the bits are a pure function of (seed, step, global
# coordinate) and the same on every backend.
_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def _mulhilo32(a: int, x):
    """(hi32, lo32) of the 64-bit product of the constant ``a`` and the 32-bit
    values ``x`` (a Python int or an int64 tensor), in 16-bit limbs of ``x`` so
    that no intermediate leaves 63 bits."""
    ph, pl = a * (x >> 16), a * (x & 0xFFFF)  # each below 2^48
    return (ph + (pl >> 16)) >> 16, (((ph & 0xFFFF) << 16) + pl) & _M32


def philox4x32_10(ctr4, key2):
    """Philox4x32-10 (the recurrence of csrc/common.h) on 32-bit values held
    in Python ints or int64 tensors: counter ``(x, y, z, w)`` and key
    ``(k0, k1)`` -> the four output words."""
    x, y, z, w = ctr4
    k0, k1 = key2
    for _ in range(10):
        hi0, lo0 = _mulhilo32(_PHILOX_M0, x)
        hi1, lo1 = _mulhilo32(_PHILOX_M1, z)
        x, y, z, w = hi1 ^ y ^ k0, lo1, hi0 ^ w ^ k1, lo0
        k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
    return x, y, z, w


def stoc_unit(coords: torch.Tensor, seed: int, step: int) -> torch.Tensor:
    """fp32 uniforms in [0, 1) of the global coordinates ``coords`` (int64).

    Coordinate c takes word ``c & 3`` of the counter ``(lo32(c8), hi32(c8),
    step & 0xFFFFFFFF, (c & 7) >> 2)`` with ``c8 = c & ~7`` under the key
    ``(lo32(seed), hi32(seed))``, as ``float(word >> 8) * 2^-24``: the
    kernel's lane layout (8 coordinates per lane from two Philox calls).  A
    lane starts at a multiple of 8 because every tensor's bits start at a
    multiple of 2048 above a coordinate base that is a multiple of 8."""
    c = coords.to(torch.int64).reshape(-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c8 = c & ~7
    words = philox4x32_10((c8 & _M32, (c8 >> 32) & _M32, torch.full_like(c, int(step) & _M32), (c & 7) >> 2),
                          (seed & _M32, seed >> 32))
    word = torch.stack(words).gather(0, (c & 3).unsqueeze(0)).squeeze(0)
    return (word >> 8).to(torch.float32) * 2.0 ** -24


def interp_exact(grad: torch.Tensor, exp_avg: torch.Tensor, beta1: float) -> torch.Tensor:
    """The kernels' expression of :func:`interp`, in the tensors' dtype:
    ``rnd(fma32(g, fp32(1 - beta1), rnd(fp32(m) * fp32(beta1))))`` with ``rnd``
    the rounding to the dtype (the identity for fp32)."""
    dt = grad.dtype
    b1 = torch.tensor(beta1, dtype=torch.float32, device=grad.device)
    mb = (exp_avg.float() * b1).to(dt).float()
    return _fma32(1 - beta1, grad.float(), mb).to(dt)


def stochastic_bits_exact(grad, exp_avg, beta1: float, rr: float, coords: torch.Tensor, seed: int,
                          step: int) -> torch.Tensor:
    """K3's vote bits, exactly: ``stoc_unit(coords) < clamp((u + rr) * (0.5 /
    rr), 0, 1)`` with ``u = interp_exact(g, m, beta1)`` and every op in fp32
    (``rr`` rounded to fp32 first; an add then a multiply, no fma).  A NaN
    ``u`` gives 0, +inf gives 1, -inf gives 0.  ``coords``: the elements'
    global coordinates, the first one a multiple of 8 (a lane boundary)."""
    c = coords.to(torch.int64).reshape(-1)
    assert c.numel() == grad.numel() and (c.numel() == 0 or int(c[0]) % 8 == 0), "a tensor starts on a lane boundary"
    u = interp_exact(grad, exp_avg, beta1).float().reshape(-1)
    rr32 = torch.tensor(rr, dtype=torch.float32, device=u.device)
    inv = torch.tensor(0.5, dtype=torch.float32, device=u.device) / rr32
    pr = ((u + rr32) * inv).clamp(0.0, 1.0)
    return (stoc_unit(c, seed, step).to(u.device) < pr).view(grad.shape)


# ------------------------------------------- reference-compatible functions
def update_fn(p, grad, exp_avg, lr, wd, beta1, beta2, rounding: int = ROUND_NEAREST,
              coords: Optional[torch.Tensor] = None, seed: int = 0, step: int = 0) -> None:
    """Single-node Lion step (ref :47-59); sign(0) leaves the coordinate.
    ``rounding`` / ``coords`` / ``seed`` / ``step``: as in :func:`apply_delta_`."""
    if _stochastic(p, rounding):
        _apply_stochastic_(p, interp(grad, exp_avg, beta1).sign_(), lr, wd, coords, seed, step)
    else:
        p.mul_(1 - lr * wd)
        p.add_(interp(grad, exp_avg, beta1).sign_(), alpha=-lr)
    momentum_update_(grad, exp_avg, beta2)


def _gather_vote(bits: torch.Tensor, shape, group, wire_dtype, tie: int) -> torch.Tensor:
    packed = pack_bits(bits)
    if wire_dtype != torch.uint8:
        packed = packed.to(wire_dtype)  # int64 reproduces the reference payload (1 B/param)
    world = dist.get_world_size(group)
    bufs = [torch.empty_like(packed) for _ in range(world)]
    dist.all_gather(bufs, packed, group=group)
    n = bits.numel()
    planes = [unpack_bits(b.to(torch.uint8), n) for b in bufs]
    return majority_vote(planes, tie=tie).view(shape)


def update_fn_distributed(p, grad, exp_avg, lr, wd, beta1, beta2, group=None, wire_dtype=torch.uint8,
                          tie: int = TIE_NEGATIVE) -> None:
    """Per-tensor distributed majority-vote step (ref :61-96 semantics)."""
    p.mul_(1 - lr * wd)
    vote = _gather_vote(sign_bits(grad, exp_avg, beta1), p.shape, group, wire_dtype, tie)
    p.add_(vote.to(torch.int8) * 2 - 1, alpha=-lr)
    momentum_update_(grad, exp_avg, beta2)


def update_fn_distributed_stoc(p, grad, exp_avg, lr, wd, beta1, beta2, max_grad_norm, group=None,
                               wire_dtype=torch.uint8, generator=None, tie: int = TIE_NEGATIVE) -> None:
    """Stochastic-binarization variant (ref :98-136 semantics, D2-D4 fixed)."""
    p.mul_(1 - lr * wd)
    bits = stochastic_bits(grad, exp_avg, beta1, max_grad_norm, generator)
    vote = _gather_vote(bits, p.shape, group, wire_dtype, tie)
    p.add_(vote.to(torch.int8) * 2 - 1, alpha=-lr)
    momentum_update_(grad, exp_avg, beta2)
