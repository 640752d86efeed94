"""Cases, references and checks shared by tests/test_kv8_gpu.py and tests/test_kv8_cpu.py (docs/TEST_TOLERANCES.md
"FP8 KV cache").  The geometry is decode_cases' / chunk_cases'.

cached_attention_fp8: the reference of query (b, t), t < n_new[b], is row len + t of numerics.attention_ref64 on the
DEQUANTISED cache rows [0, len + n) (fused.kv_dequantize: code * scale, exact) with the chunk's queries placed at
their rows; the rounding model is the same call with model=True; the bound is assert_rows_close at the existing
C_ROWS.  Every code at or beyond len[b] + n_new[b] is 0x7F (e4m3 NaN) and every such scale NaN, so finite outputs
prove that neither is read or multiplied in.  Queries t >= n_new[b] must be zero rows.

The quantising writers: codes and scales are bit-equal to fused.kv_quantize_reference of the bf16 rows the bf16 cache
holds (chunk_cases / decode_cases check those against fused.rope / fused.qk_norm_rope), q bit-equal to the bf16
call's, unwritten positions and the guard bands keep their poison."""
import functools

import torch

import chunk_cases as cc
import decode_cases as dc
import numerics as nm
from distributed_lion_pytorch_amd.ops import fused

B, TMAX, HEADS, DIMS, FORCED_SPLITS = dc.B, dc.TMAX, dc.HEADS, dc.DIMS, dc.FORCED_SPLITS
CHUNKS = (1, 5, 8)
TILE = 64  # csrc/kv8_attention.hip kTile: a wave's key tile
NAN_CODE, POISON_CODE, POISON_SCALE = 0x7F, 0xA5, -7.0


def length_sets(Hkv, T):
    """Base lengths whose len + T sits around the key tile, around the unforced grid's first split boundary c, and at
    0, 1 and TMAX."""
    c = cc.boundary(Hkv, T)
    return [(TILE - 1 - T, TILE - T, TILE + 1 - T), (c - 1 - T, c - T, c + 1 - T), (0, 1, TMAX - T)]


WINDOW_CASES = cc.WINDOW_CASES  # windows 1, 16 and one that covers every length
BOUND_CASES = cc.BOUND_CASES  # max_len below TMAX at T = 5


def ragged(T):
    return (0, 1, T)


@functools.lru_cache(maxsize=None)
def attention_case(D, H, Hkv, T, lens, n_new=None, window=0, max_len=None, seed=0):
    """CPU tensors of one case: q [B, T, H, D] bf16, codes [B, TMAX, Hkv, D] / scales [B, TMAX, Hkv] of k and v with
    NaN codes and scales at and beyond len + n_new, kv_len / n_new int32 [B], ref64 / model [B, T, H D]."""
    g = torch.Generator().manual_seed(2000 * D + 10 * H + Hkv + 7 * T + seed)
    q = torch.randn(B, T, H, D, generator=g).to(torch.bfloat16)
    # rows of different magnitudes, so that the scales differ from key to key
    mag = torch.exp2(4 * torch.rand(B, TMAX, Hkv, 1, generator=g) - 2)
    kc, ks = fused.kv_quantize_reference((torch.randn(B, TMAX, Hkv, D, generator=g) * mag).to(torch.bfloat16))
    vc, vs = fused.kv_quantize_reference((torch.randn(B, TMAX, Hkv, D, generator=g) * mag.flip(1)).to(torch.bfloat16))
    ns = (T,) * B if n_new is None else tuple(n_new)
    ref = torch.zeros(B, T, H * D, dtype=torch.float64)
    model = torch.zeros(B, T, H * D, dtype=torch.float64)
    cap = TMAX if max_len is None else max_len
    live = []
    for b, (base, n) in enumerate(zip(lens, ns)):
        base = min(base, cap)
        n = min(n, cap - base)
        live.append(n)
        L = base + n
        assert 0 <= base and L <= TMAX
        for codes, scales in ((kc, ks), (vc, vs)):
            codes[b, L:] = NAN_CODE
            scales[b, L:] = float("nan")
        if n == 0:
            continue
        k, v = fused.kv_dequantize(kc[b:b + 1, :L], ks[b:b + 1, :L]), fused.kv_dequantize(vc[b:b + 1, :L], vs[b:b + 1, :L])
        qq = torch.zeros(1, L, H, D, dtype=torch.bfloat16)
        qq[0, base:L] = q[b, :n]
        dout = torch.zeros(1, L, H * D)
        for out, is_model in ((ref, False), (model, True)):
            out[b, :n] = nm.attention_ref64(qq, k, v, dout, 0.0, 0, window, model=is_model)[0][0, base:L]
    return dict(q=q, kc=kc, ks=ks, vc=vc, vs=vs, kv_len=torch.tensor(lens, dtype=torch.int32), ns=tuple(live), ref=ref,
                model=model, n_new=None if n_new is None else torch.tensor(ns, dtype=torch.int32))


def check_attention_case(fn, device, D, H, Hkv, T, lens, n_new=None, window=0, splits=FORCED_SPLITS, max_len=None):
    """fn = fused.cached_attention_fp8 or its PyTorch form.  Every forced split count is within the bound, two runs of
    a call are bit-identical, and queries at or beyond n_new (a row without keys among them) are zero rows."""
    c = attention_case(D, H, Hkv, T, tuple(lens), None if n_new is None else tuple(n_new), window, max_len)
    q, kc, ks, vc, vs, kv_len = (c[n].to(device) for n in ("q", "kc", "ks", "vc", "vs", "kv_len"))
    nn = None if c["n_new"] is None else c["n_new"].to(device)
    worst = 0.0
    for s in splits:
        kw = {} if s is None else {"splits": s}
        name = f"kv8 D={D} H={H}/{Hkv} T={T} lens={tuple(lens)} n_new={n_new} window={window} max_len={max_len} splits={s}"
        out = fn(q, kc, ks, vc, vs, kv_len, nn, window, max_len, **kw)
        assert out.shape == (B, T, H * D) and out.dtype == torch.bfloat16
        worst = max(worst, nm.assert_rows_close(out.cpu(), c["ref"], c["model"], nm.C_ROWS, name=name))
        nm.assert_bits(fn(q, kc, ks, vc, vs, kv_len, nn, window, max_len, **kw), out, name + " second run")
        for b, n in enumerate(c["ns"]):
            assert bool((out[b, n:] == 0).all()), name + ": a query at or beyond n_new must be a zero row"
    return worst


# ------------------------------------------------------------------------------------- the quantising writers
def guarded_cache8(D, device):
    """(codes view [B, TMAX, Hkv, D], scales view [B, TMAX, Hkv], both whole buffers): decode_cases.guarded_cache for
    the fp8 cache, all poison."""
    n = dc.APPEND_B * dc.APPEND_TMAX * dc.APPEND_HKV
    cbuf = torch.full((n * D + 2 * dc.GUARD,), POISON_CODE, dtype=torch.uint8, device=device)
    sbuf = torch.full((n + 2 * dc.GUARD,), POISON_SCALE, dtype=torch.float32, device=device)
    shape = (dc.APPEND_B, dc.APPEND_TMAX, dc.APPEND_HKV)
    return cbuf[dc.GUARD:dc.GUARD + n * D].view(*shape, D), sbuf[dc.GUARD:dc.GUARD + n].view(shape), cbuf, sbuf


def assert_cache8(name, codes, scales, cbuf, sbuf, written, expected):
    """written [B, TMAX] bool; expected bf16 [n written, Hkv, D] in row-major order of the written positions."""
    ec, es = fused.kv_quantize_reference(expected)
    nm.assert_bits(codes[written], ec, name + " codes")
    nm.assert_bits(scales[written], es, name + " scales")
    assert bool((codes[~written] == POISON_CODE).all()) and bool((scales[~written] == POISON_SCALE).all()), name + ": written outside"
    for buf, poison in ((cbuf, POISON_CODE), (sbuf, POISON_SCALE)):
        assert bool((buf[:dc.GUARD] == poison).all()) and bool((buf[-dc.GUARD:] == poison).all()), name + ": guard band"


def append_args(D, mode, device):
    _, gq, gk, cos, sin = (t.to(device) for t in dc.append_inputs(D))
    if mode == "append":
        cos = sin = None
    if mode != "norm_rope":
        gq = gk = None
    return cos, sin, gq, gk


def check_append(fn, device, D, mode):
    """fn = fused.kv_append: the fp8 stores against the bf16 call's cache rows, q against the bf16 call's q."""
    cos, sin, gq, gk = append_args(D, mode, device)
    q, k, v = dc.split_step(dc.append_inputs(D)[0].to(device), D)
    p = torch.tensor(dc.APPEND_POS, dtype=torch.int32, device=device)
    kb, vb = dc.guarded_cache(D, device)[0], dc.guarded_cache(D, device)[0]
    q_ref = fn(q, k, v, p, cos, sin, gq, gk, dc.APPEND_EPS, kb, vb)
    kc, ks, kcb, ksb = guarded_cache8(D, device)
    vc, vs, vcb, vsb = guarded_cache8(D, device)
    q_out = fn(q, k, v, p, cos, sin, gq, gk, dc.APPEND_EPS, kc, vc, ks, vs)
    name = f"kv_append fp8 D={D} {mode}"
    nm.assert_bits(q_out, q_ref, name + " q")
    written = torch.zeros(dc.APPEND_B, dc.APPEND_TMAX, dtype=torch.bool, device=device)
    written[torch.arange(dc.APPEND_B, device=device), p.long()] = True
    assert_cache8(name + " k", kc, ks, kcb, ksb, written, kb[written])
    assert_cache8(name + " v", vc, vs, vcb, vsb, written, vb[written])


def check_append_chunk(fn, device, D, T, mode):
    """fn = fused.kv_append_chunk, ragged by n_new (chunk_cases.append_positions)."""
    cos, sin, gq, gk = append_args(D, mode, device)
    q, k, v = cc.split_chunk(cc.append_inputs(D, T).to(device), D)
    pos, ns = cc.append_positions(T)
    p = torch.tensor(pos, dtype=torch.int32, device=device)
    nn = torch.tensor(ns, dtype=torch.int32, device=device)
    kb, vb = dc.guarded_cache(D, device)[0], dc.guarded_cache(D, device)[0]
    q_ref = fn(q, k, v, p, cos, sin, gq, gk, dc.APPEND_EPS, kb, vb, nn)
    kc, ks, kcb, ksb = guarded_cache8(D, device)
    vc, vs, vcb, vsb = guarded_cache8(D, device)
    q_out = fn(q, k, v, p, cos, sin, gq, gk, dc.APPEND_EPS, kc, vc, nn, ks, vs)
    name = f"kv_append_chunk fp8 D={D} T={T} {mode}"
    written = torch.zeros(dc.APPEND_B, dc.APPEND_TMAX, dtype=torch.bool, device=device)
    for b in range(dc.APPEND_B):
        nm.assert_bits(q_out[b, :ns[b]], q_ref[b, :ns[b]], f"{name} q row {b}")
        written[b, pos[b]:pos[b] + ns[b]] = True
    assert_cache8(name + " k", kc, ks, kcb, ksb, written, kb[written])
    assert_cache8(name + " v", vc, vs, vcb, vsb, written, vb[written])


def hand_rows():
    """bf16 rows [n, 64] for the quantiser's corners, by name."""
    def row(first, rest=0.0):
        r = torch.full((64,), rest, dtype=torch.float32)
        r[:len(first)] = torch.tensor(first, dtype=torch.float32)
        return r.to(torch.bfloat16)

    return {
        "zeros": row([0.0]),
        "absmax 1.75": row([1.75, -1.0]),  # e = -7: 1.75 / 2^-7 = 224
        "absmax below 1.75": row([1.7421875, 1.0]),  # the bf16 below 1.75: e = -8, 446
        # scale 2^-8: 2^-17 is the smallest subnormal code, 2^-18 a tie to zero, 3 2^-18 a tie to even (2^-16);
        # 17 / 2^12 lies between the codes 16 / 2^12 and 18 / 2^12: a tie to even in a normal binade
        "subnormal codes and ties": row([1.0, 2.0 ** -17, 2.0 ** -18, 3 * 2.0 ** -18, -2.0 ** -18, 17 / 4096, 19 / 4096]),
        "negative zero": row([1.0, -0.0]),
        "absmax 2^-120": row([2.0 ** -120, -2.0 ** -124, 2.0 ** -130]),  # e clamps at -126
        "absmax 2^-117": row([2.0 ** -117, 2.0 ** -126]),
        "absmax 2^120": row([-2.0 ** 120, 2.0 ** 112, 1.0]),
    }
