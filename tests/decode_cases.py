"""Cases, references and checks shared by tests/test_decode_attention_gpu.py, tests/test_kv_append_gpu.py and
the PyTorch-form checks of tests/test_generate_cpu.py (docs/TEST_TOLERANCES.md "Generation").

decode_attention: row b's reference is the last query row of numerics.attention_ref64 on q, k_cache[b, :len],
v_cache[b, :len] with T = len, p = 0 and the case's window; the rounding model is the same call with
model=True; the bound is assert_rows_close at the existing C_ROWS.  Every cache element at or beyond kv_len[b]
is NaN, so a finite output proves that nothing beyond the length is read or multiplied in.

kv_append: the rotated q and the appended k are bit-equal to row pos[b] of fused.rope / fused.qk_norm_rope on
a [B, T, H, D] tensor holding the same token at that position."""
import functools

import torch

import numerics as nm
from distributed_lion_pytorch_amd.models.llama import Rotary
from distributed_lion_pytorch_amd.ops import fused

B = 3
TMAX = 520
HEADS = [(4, 4), (8, 2), (7, 1), (8, 1)]
DIMS = [64, 128]
FORCED_SPLITS = (None, 1, 2, fused._DECODE_MAX_SPLITS)


def boundary(Hkv, max_len=TMAX, window=0):
    """The first split boundary of the kernel's own (unforced) grid for these cases."""
    splits, chunk = fused.decode_splits(B, Hkv, max_len, window)
    assert splits >= 2, "the cases are meant to cross a split boundary of the unforced grid"
    return chunk


def length_sets(Hkv):
    c = boundary(Hkv)
    return [(1, 64, TMAX), (2, 63, 65), (c - 1, c, c + 1), (2 * c - 1, 2 * c + 1, 0)]


# (window, lengths): 1, 16 and a window that covers every length
WINDOW_CASES = [(1, (1, 65, 300)), (16, (15, 16, 17)), (16, (2, 64, TMAX)), (TMAX + 7, (63, 300, TMAX))]


@functools.lru_cache(maxsize=None)
def attention_case(D, H, Hkv, lens, window=0, max_len=None, seed=0):
    """CPU tensors of one case: qkv [B, (H + 2 Hkv) D] (q is its first H D columns), caches [B, TMAX, Hkv, D]
    with NaN at and beyond each row's length, kv_len int32 [B] (a length above max_len is given as it is: the op
    clamps it), ref64 / model [B, H D]."""
    g = torch.Generator().manual_seed(1000 * D + 10 * H + Hkv + seed)
    qkv = torch.randn(B, (H + 2 * Hkv) * D, generator=g).to(torch.bfloat16)
    k = torch.randn(B, TMAX, Hkv, D, generator=g).to(torch.bfloat16)
    v = torch.randn(B, TMAX, Hkv, D, generator=g).to(torch.bfloat16)
    ref = torch.zeros(B, H * D, dtype=torch.float64)
    model = torch.zeros(B, H * D, dtype=torch.float64)
    for b, n_given in enumerate(lens):
        n = min(n_given, TMAX if max_len is None else max_len)
        k[b, n:] = float("nan")
        v[b, n:] = float("nan")
        if n == 0:
            continue  # no keys: a zero row
        q = qkv[b, :H * D].view(1, 1, H, D).expand(1, n, H, D)
        dout = torch.zeros(1, n, H * D)
        for out, is_model in ((ref, False), (model, True)):
            out[b] = nm.attention_ref64(q, k[b:b + 1, :n], v[b:b + 1, :n], dout, 0.0, 0, window, model=is_model)[0][0, -1]
    return dict(qkv=qkv, k=k, v=v, kv_len=torch.tensor(lens, dtype=torch.int32), ref=ref, model=model)


def check_attention_case(fn, device, D, H, Hkv, lens, window=0, max_len=None, splits=FORCED_SPLITS, shared_cache=False):
    """fn = fused.decode_attention or its PyTorch form.  Every forced split count is within the bound, and two
    runs of a call are bit-identical.  shared_cache: k and v are the two halves of one [B, TMAX, 2, Hkv, D] buffer
    (token stride 2 Hkv D)."""
    c = attention_case(D, H, Hkv, tuple(lens), window, max_len)
    qkv = c["qkv"].to(device)
    q = qkv[:, :H * D].view(B, H, D)  # a strided view of the packed q|k|v rows
    assert not q.is_contiguous()
    if shared_cache:
        kv = torch.stack([c["k"], c["v"]], dim=2).to(device)
        k, v = kv[:, :, 0], kv[:, :, 1]
    else:
        k, v = c["k"].to(device), c["v"].to(device)
    kv_len = c["kv_len"].to(device)
    worst = 0.0
    for s in splits:
        kw = {} if s is None else {"splits": s}
        name = f"decode D={D} H={H}/{Hkv} lens={tuple(lens)} window={window} max_len={max_len} splits={s}"
        out = fn(q, k, v, kv_len, window, max_len, **kw)
        assert out.shape == (B, H * D) and out.dtype == torch.bfloat16
        worst = max(worst, nm.assert_rows_close(out.cpu(), c["ref"], c["model"], nm.C_ROWS, name=name))
        nm.assert_bits(fn(q, k, v, kv_len, window, max_len, **kw), out, name + " second run")
        for b, n in enumerate(lens):
            if n == 0:
                assert bool((out[b] == 0).all()), name + ": a row without keys must be zero"
    return worst


# ------------------------------------------------------------------------------------------- kv_append
APPEND_B, APPEND_H, APPEND_HKV, APPEND_TMAX, APPEND_EPS = 4, 4, 2, 33, 1e-6
APPEND_POS = (0, APPEND_TMAX - 1, 7, 20)
POISON = -1234.0  # exact in bf16
GUARD = 4096  # elements on either side of a cache


@functools.lru_cache(maxsize=None)
def append_inputs(D, seed=0):
    g = torch.Generator().manual_seed(77 + D + seed)
    Hx = APPEND_H + 2 * APPEND_HKV
    qkv = torch.randn(APPEND_B, Hx * D, generator=g).to(torch.bfloat16)
    gq = (1 + 0.25 * torch.randn(D, generator=g)).to(torch.bfloat16)
    gk = (1 + 0.25 * torch.randn(D, generator=g)).to(torch.bfloat16)
    cos, sin = Rotary(D, 10000.0).tables(APPEND_TMAX, torch.device("cpu"), torch.bfloat16)
    return qkv, gq, gk, cos, sin


def guarded_cache(D, device):
    """(cache view [B, TMAX, Hkv, D], whole buffer): the cache sits between two guard bands, all poison."""
    n = APPEND_B * APPEND_TMAX * APPEND_HKV * D
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.bfloat16, device=device)
    return buf[GUARD:GUARD + n].view(APPEND_B, APPEND_TMAX, APPEND_HKV, D), buf


def split_step(qkv, D):
    H, Hkv = APPEND_H, APPEND_HKV
    n = qkv.shape[0]
    return (qkv[:, :H * D].view(n, H, D), qkv[:, H * D:(H + Hkv) * D].view(n, Hkv, D),
            qkv[:, (H + Hkv) * D:].view(n, Hkv, D))


def expected_rows(x, pos, cos, sin, gamma):
    """Row pos[b] of fused.rope / fused.qk_norm_rope on a [B, T, heads, D] tensor that holds x[b] at that position."""
    n, Hx, D = x.shape
    full = torch.zeros(n, APPEND_TMAX, Hx, D, dtype=x.dtype, device=x.device)
    rows = torch.arange(n, device=x.device)
    p = torch.tensor(pos, device=x.device)
    full[rows, p] = x
    y = fused.rope(full, cos, sin) if gamma is None else fused.qk_norm_rope(full, gamma, APPEND_EPS, cos, sin)
    return y[rows, p]


def check_append(fn, device, D, gains, tables=True, pos=APPEND_POS):
    """fn = fused.kv_append or its PyTorch form, at in-range positions."""
    qkv, gq, gk, cos, sin = (t.to(device) for t in append_inputs(D))
    q, k, v = split_step(qkv, D)
    if not tables:
        cos = sin = None
    if not gains:
        gq = gk = None
    kc, kbuf = guarded_cache(D, device)
    vc, vbuf = guarded_cache(D, device)
    name = f"kv_append D={D} gains={gains} tables={tables}"
    p = torch.tensor(pos, dtype=torch.int32, device=device)
    q_out = fn(q, k, v, p, cos, sin, gq, gk, APPEND_EPS, kc, vc)
    assert q_out.shape == q.shape and q_out.is_contiguous()
    if tables:
        exp_q, exp_k = expected_rows(q, pos, cos, sin, gq), expected_rows(k, pos, cos, sin, gk)
    else:
        exp_q, exp_k = q, k
    nm.assert_bits(q_out, exp_q.contiguous(), name + " q")
    rows = torch.arange(APPEND_B, device=device)
    pl = p.long()
    nm.assert_bits(kc[rows, pl], exp_k.contiguous(), name + " appended k")
    nm.assert_bits(vc[rows, pl], v.contiguous(), name + " appended v")
    for cache, buf, what in ((kc, kbuf, "k"), (vc, vbuf, "v")):
        untouched = torch.ones(cache.shape[:2], dtype=torch.bool, device=device)
        untouched[rows, pl] = False
        assert bool((cache[untouched] == POISON).all()), f"{name}: {what} cache written outside cache[b, pos[b]]"
        assert bool((buf[:GUARD] == POISON).all()) and bool((buf[-GUARD:] == POISON).all()), f"{name}: {what} guard band"
