"""Cases, references and checks shared by tests/test_chunk_attention_gpu.py, tests/test_kv_append_chunk_gpu.py and
the PyTorch-form checks of tests/test_speculative_cpu.py (docs/TEST_TOLERANCES.md "Chunk attention / speculative
decoding").  The geometry is decode_cases'.

chunk_attention: query (b, t), t < n_new[b], has as reference row len + t of numerics.attention_ref64 on
k_cache[b, :len + n], v_cache[b, :len + n] with the chunk's queries placed at their rows (p = 0, the case's
window); the rounding model is the same call with model=True; the bound is assert_rows_close at the existing
C_ROWS.  Queries t >= n_new[b] must be zero rows.  Every cache element at or beyond len[b] + n_new[b] is NaN, so
finite outputs prove that nothing beyond is read or multiplied in.

kv_append_chunk: the rotated q and the appended k are bit-equal to rows pos[b] + t of fused.rope /
fused.qk_norm_rope on a [B, Tmax, heads, D] tensor holding the chunk's tokens at those positions."""
import functools

import torch

import decode_cases as dc
import numerics as nm
from distributed_lion_pytorch_amd.ops import fused

B, TMAX, HEADS, DIMS, FORCED_SPLITS = dc.B, dc.TMAX, dc.HEADS, dc.DIMS, dc.FORCED_SPLITS
CHUNKS = (1, 2, 5, 8)


def boundary(Hkv, T, window=0):
    """The first split boundary of the kernel's own (unforced) grid for these cases."""
    splits, chunk = fused.chunk_splits(B, Hkv, TMAX, T, window)
    assert splits >= 2, "the cases are meant to cross a split boundary of the unforced grid"
    return chunk


def length_sets(Hkv, T):
    """Base lengths whose len + T straddles 64, the first split boundary c and its multiple, and ends at TMAX."""
    c = boundary(Hkv, T)
    return [(1, 63, c - 2), (c - T, 2 * c - 1, TMAX - T)]


# (window, base lengths): 1, 16 and a window that covers every length
WINDOW_CASES = [(1, (0, 65, 300)), (16, (10, 15, 16)), (16, (2, 64, 400)), (TMAX + 7, (63, 300, 400))]


# (base lengths, max_len) at T = 5: a host bound just above the longest row (two splits of the unforced grid), and one
# that a row exceeds (clamped: it keeps no token)
BOUND_CASES = [((5, 200, 300), 305), ((5, 200, 300), 250), ((60, 248, 100), 250)]


def ragged(T):
    return (0, 1, T)


@functools.lru_cache(maxsize=None)
def attention_case(D, H, Hkv, T, lens, n_new=None, window=0, max_len=None, seed=0):
    """CPU tensors of one case: q [B, T, H, D], caches [B, TMAX, Hkv, D] with NaN at and beyond len + n_new,
    kv_len / n int32 [B], ref64 / model [B, T, H D] (zero rows for t >= n_new[b]).  max_len: the host bound on
    len + n_new; a row beyond it is given as it is and the op clamps it (len to max_len, n_new to what is left)."""
    g = torch.Generator().manual_seed(1000 * D + 10 * H + Hkv + 7 * T + seed)
    q = torch.randn(B, T, H, D, generator=g).to(torch.bfloat16)
    k = torch.randn(B, TMAX, Hkv, D, generator=g).to(torch.bfloat16)
    v = torch.randn(B, TMAX, Hkv, D, generator=g).to(torch.bfloat16)
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
        assert L <= TMAX
        k[b, L:] = float("nan")
        v[b, L:] = float("nan")
        if n == 0:
            continue
        qq = torch.zeros(1, L, H, D, dtype=torch.bfloat16)
        qq[0, base:L] = q[b, :n]
        dout = torch.zeros(1, L, H * D)
        for out, is_model in ((ref, False), (model, True)):
            out[b, :n] = nm.attention_ref64(qq, k[b:b + 1, :L], v[b:b + 1, :L], dout, 0.0, 0, window, model=is_model)[0][0, base:L]
    return dict(q=q, k=k, v=v, kv_len=torch.tensor(lens, dtype=torch.int32), ns=tuple(live), ref=ref, model=model,
                n_new=None if n_new is None else torch.tensor(ns, dtype=torch.int32))


def check_attention_case(fn, device, D, H, Hkv, T, lens, n_new=None, window=0, splits=FORCED_SPLITS, shared_cache=False,
                         max_len=None):
    """fn = fused.chunk_attention or its PyTorch form.  Every forced split count is within the bound, and two runs
    of a call are bit-identical.  shared_cache: k and v are the two halves of one [B, TMAX, 2, Hkv, D] buffer."""
    c = attention_case(D, H, Hkv, T, tuple(lens), None if n_new is None else tuple(n_new), window, max_len)
    q = c["q"].to(device)
    if shared_cache:
        kv = torch.stack([c["k"], c["v"]], dim=2).to(device)
        k, v = kv[:, :, 0], kv[:, :, 1]
    else:
        k, v = c["k"].to(device), c["v"].to(device)
    kv_len = c["kv_len"].to(device)
    nn = None if c["n_new"] is None else c["n_new"].to(device)
    worst = 0.0
    for s in splits:
        kw = {} if s is None else {"splits": s}
        name = f"chunk D={D} H={H}/{Hkv} T={T} lens={tuple(lens)} n_new={n_new} window={window} max_len={max_len} splits={s}"
        out = fn(q, k, v, kv_len, nn, window, max_len, **kw)
        assert out.shape == (B, T, H * D) and out.dtype == torch.bfloat16
        worst = max(worst, nm.assert_rows_close(out.cpu(), c["ref"], c["model"], nm.C_ROWS, name=name))
        nm.assert_bits(fn(q, k, v, kv_len, nn, window, max_len, **kw), out, name + " second run")
        for b, n in enumerate(c["ns"]):
            assert bool((out[b, n:] == 0).all()), name + ": a query at or beyond n_new must be a zero row"
    return worst


# ------------------------------------------------------------------------------------- kv_append_chunk
MODES = ("append", "rope", "norm_rope")


@functools.lru_cache(maxsize=None)
def append_inputs(D, T, seed=0):
    g = torch.Generator().manual_seed(91 + D + 3 * T + seed)
    Hx = dc.APPEND_H + 2 * dc.APPEND_HKV
    return torch.randn(dc.APPEND_B, T, Hx * D, generator=g).to(torch.bfloat16)


def split_chunk(qkv, D):
    H, Hkv = dc.APPEND_H, dc.APPEND_HKV
    n, T = qkv.shape[:2]
    return (qkv[..., :H * D].view(n, T, H, D), qkv[..., H * D:(H + Hkv) * D].view(n, T, Hkv, D),
            qkv[..., (H + Hkv) * D:].view(n, T, Hkv, D))


def append_positions(T):
    """(pos, n_new): row 0 ends exactly at TMAX - 1, row 1 keeps nothing, row 2 is ragged, row 3 starts at 0."""
    return (dc.APPEND_TMAX - T, 5, 7, 0), (T, 0, max(1, T - 1), T)


def expected_chunk(x, pos, cos, sin, gamma):
    """Rows pos[b] + t of fused.rope / fused.qk_norm_rope on a [B, TMAX, heads, D] tensor that holds x[b, t] there;
    every token's position, live or dead, must lie inside the cache."""
    n, T, Hx, D = x.shape
    full = torch.zeros(n, dc.APPEND_TMAX, Hx, D, dtype=x.dtype, device=x.device)
    rows = torch.arange(n, device=x.device)[:, None].expand(n, T)
    p = torch.tensor(pos, device=x.device)[:, None] + torch.arange(T, device=x.device)[None, :]
    assert 0 <= int(p.min()) and int(p.max()) < dc.APPEND_TMAX
    full[rows, p] = x
    y = fused.rope(full, cos, sin) if gamma is None else fused.qk_norm_rope(full, gamma, dc.APPEND_EPS, cos, sin)
    return y[rows, p]


def check_append_chunk(fn, device, D, T, mode):
    """fn = fused.kv_append_chunk or its PyTorch form, at in-range positions with a ragged n_new."""
    _, gq, gk, cos, sin = (t.to(device) for t in dc.append_inputs(D))
    qkv = append_inputs(D, T).to(device)
    q, k, v = split_chunk(qkv, D)
    if mode == "append":
        cos = sin = None
    if mode != "norm_rope":
        gq = gk = None
    pos, ns = append_positions(T)
    kc, kbuf = dc.guarded_cache(D, device)
    vc, vbuf = dc.guarded_cache(D, device)
    name = f"kv_append_chunk D={D} T={T} {mode}"
    p = torch.tensor(pos, dtype=torch.int32, device=device)
    nn = torch.tensor(ns, dtype=torch.int32, device=device)
    q_out = fn(q, k, v, p, cos, sin, gq, gk, dc.APPEND_EPS, kc, vc, nn)
    assert q_out.shape == q.shape and q_out.is_contiguous()
    if mode == "append":
        exp_q, exp_k = q, k
    else:
        exp_q, exp_k = expected_chunk(q, pos, cos, sin, gq), expected_chunk(k, pos, cos, sin, gk)
    untouched = torch.ones(dc.APPEND_B, dc.APPEND_TMAX, dtype=torch.bool, device=device)
    for b in range(dc.APPEND_B):
        n = ns[b]
        nm.assert_bits(q_out[b, :n], exp_q[b, :n].contiguous(), f"{name} q row {b}")
        nm.assert_bits(kc[b, pos[b]:pos[b] + n], exp_k[b, :n].contiguous(), f"{name} appended k row {b}")
        nm.assert_bits(vc[b, pos[b]:pos[b] + n], v[b, :n].contiguous(), f"{name} appended v row {b}")
        untouched[b, pos[b]:pos[b] + n] = False
    for cache, buf, what in ((kc, kbuf, "k"), (vc, vbuf, "v")):
        assert bool((cache[untouched] == dc.POISON).all()), f"{name}: {what} cache written outside the live tokens"
        assert bool((buf[:dc.GUARD] == dc.POISON).all()) and bool((buf[-dc.GUARD:] == dc.POISON).all()), f"{name}: {what} guard band"
