"""fused.shared_prefix_attention and fused.kv_append_suffix (csrc/prefix_attention.hip).

Attention: beam row r = b * nb + j against the last query row of numerics.attention_ref64 over prompt b's prefix keys
followed by the row's own suffix keys (T = their number, p = 0, the case's window), its model=True twin as the rounding
model, numerics.assert_rows_close at the existing C_ROWS -- the check of tests/decode_cases.py.  Both caches hold NaN at
and beyond their (clamped) lengths, so a finite output proves nothing beyond a length was read.  Lengths sit on either
side of the 16- / 32-key tiles and of the unforced grid's first split boundary; R = nb * H / Hkv is 2, 16, 21 and 64.

Append: q and the appended k are bit-equal to fused.kv_append at the same absolute position, v is copied, nothing else
in a guarded suffix cache is written; a write position outside the cache raises and writes nothing."""
import functools

import pytest
import torch

import decode_cases as dc
import numerics as nm
from distributed_lion_pytorch_amd.ops import fused, hip

pytestmark = pytest.mark.gpu

BP, TP, TS = 2, 258, 40
BEAM_HEADS = [(2, 4, 4), (4, 8, 2), (3, 7, 1), (8, 8, 1)]  # (nb, H, Hkv): R = 2, 16, 21, 64
SUFFIX = (1, 33, 7, 16, 32, 2, 17, 40)  # ragged suffix lengths, row r takes SUFFIX[r % 8]
MAXIMA = (fused._DECODE_MAX_SPLITS, fused._DECODE_MAX_SPLITS)
FORCED = ((1, 1), (2, 1), MAXIMA, None)
# (window, max_prefix, max_suffix): inside the prefix; per row inside / hiding it; hiding it for every row (neutral
# prefix partials); wider than everything; host bounds below the lengths, without and with a window
BOUNDED = [(40, None, None), (8, None, None), (1, None, None), (TP + TS + 7, None, None), (0, 100, 20), (30, 100, 20)]


def prefix_lengths(Hkv):
    (s1, c), _ = fused.shared_prefix_splits(BP, 2, Hkv, TP, TS)
    assert s1 >= 2, "the cases are meant to cross a split boundary of the unforced grid"
    return [(1, 33), (63, 65), (c - 1, c + 1)]


@functools.lru_cache(maxsize=None)
def case(D, nb, H, Hkv, plens, window=0, max_prefix=None, max_suffix=None):
    """CPU tensors of one case; the references run on the lengths clamped to the host bounds."""
    rows = BP * nb
    g = torch.Generator().manual_seed(1000 * D + 10 * H + nb)
    qkv = torch.randn(rows, (H + 2 * Hkv) * D, generator=g).to(torch.bfloat16)
    kp, vp = (torch.randn(BP, TP, Hkv, D, generator=g).to(torch.bfloat16) for _ in range(2))
    ks, vs = (torch.randn(rows, TS, Hkv, D, generator=g).to(torch.bfloat16) for _ in range(2))
    slens = [SUFFIX[r % len(SUFFIX)] for r in range(rows)]
    pc = [min(n, max_prefix or TP) for n in plens]
    sc = [min(n, max_suffix or TS) for n in slens]
    for b, n in enumerate(pc):
        kp[b, n:], vp[b, n:] = float("nan"), float("nan")
    ref, model = torch.zeros(rows, H * D, dtype=torch.float64), torch.zeros(rows, H * D, dtype=torch.float64)
    for r, ns in enumerate(sc):
        ks[r, ns:], vs[r, ns:] = float("nan"), float("nan")
        b = r // nb
        k = torch.cat([kp[b:b + 1, :pc[b]], ks[r:r + 1, :ns]], dim=1)
        v = torch.cat([vp[b:b + 1, :pc[b]], vs[r:r + 1, :ns]], dim=1)
        n = k.shape[1]
        q = qkv[r, :H * D].view(1, 1, H, D).expand(1, n, H, D)
        for out, is_model in ((ref, False), (model, True)):
            out[r] = nm.attention_ref64(q, k, v, torch.zeros(1, n, H * D), 0.0, 0, window, model=is_model)[0][0, -1]
    i32 = dict(dtype=torch.int32)
    return dict(qkv=qkv, kp=kp, vp=vp, ks=ks, vs=vs, plen=torch.tensor(plens, **i32), slen=torch.tensor(slens, **i32),
                ref=ref, model=model)


def check(dev, D, nb, H, Hkv, plens, window=0, max_prefix=None, max_suffix=None, forced=FORCED):
    c = {k: v.to(dev) if k not in ("ref", "model") else v
         for k, v in case(D, nb, H, Hkv, tuple(plens), window, max_prefix, max_suffix).items()}
    q = c["qkv"][:, :H * D].view(BP * nb, H, D)  # a strided view of the packed q|k|v rows
    args = (q, c["kp"], c["vp"], c["plen"], c["ks"], c["vs"], c["slen"], nb, window, max_prefix, max_suffix)
    for s in forced:
        name = f"prefix D={D} nb={nb} H={H}/{Hkv} plens={plens} window={window} bounds={max_prefix, max_suffix} splits={s}"
        out = fused.shared_prefix_attention(*args, splits=s)
        assert out.shape == (BP * nb, H * D) and out.dtype == torch.bfloat16
        nm.assert_rows_close(out.cpu(), c["ref"], c["model"], nm.C_ROWS, name=name)  # prints the case's max ratio
        nm.assert_bits(fused.shared_prefix_attention(*args, splits=s), out, name + " second run")


@pytest.fixture
def kernel_only(monkeypatch):
    hip.require()
    for f in ("shared_prefix_attention_reference", "kv_append_suffix_reference"):
        monkeypatch.setattr(fused, f, lambda *a, **kw: pytest.fail("the PyTorch form ran"))


@pytest.mark.parametrize("nb,H,Hkv", BEAM_HEADS, ids=[f"{nb}x{H}/{k}" for nb, H, k in BEAM_HEADS])
@pytest.mark.parametrize("D", [64, 128])
def test_lengths_and_splits(D, nb, H, Hkv, cuda, kernel_only):
    for plens in prefix_lengths(Hkv):
        check(cuda, D, nb, H, Hkv, plens)


@pytest.mark.parametrize("window,max_prefix,max_suffix", BOUNDED)
@pytest.mark.parametrize("D", [64, 128])
def test_windows_and_host_bounds(D, window, max_prefix, max_suffix, cuda, kernel_only):
    for nb, H, Hkv in ((3, 7, 1), (4, 8, 2)):
        check(cuda, D, nb, H, Hkv, (63, 130), window, max_prefix, max_suffix, forced=((2, 2), None))


ROT = (0, dc.APPEND_TMAX - 1, 7, 20)  # the absolute positions (the tables' rows)
WRITE = (3, 0, dc.APPEND_TMAX - 1, 11)  # the suffix indices


@pytest.mark.parametrize("gains,tables", [(False, False), (False, True), (True, True)])
@pytest.mark.parametrize("D", [64, 128])
def test_append_suffix_equals_kv_append(D, gains, tables, cuda, kernel_only):
    qkv, gq, gk, cos, sin = (t.to(cuda) for t in dc.append_inputs(D))
    q, k, v = dc.split_step(qkv, D)
    cos, sin = (cos, sin) if tables else (None, None)
    gq, gk = (gq, gk) if gains else (None, None)
    rot, wr = (torch.tensor(p, dtype=torch.int32, device=cuda) for p in (ROT, WRITE))
    (kc, kbuf), (vc, vbuf), (kr, _), (vr, _) = (dc.guarded_cache(D, cuda) for _ in range(4))
    q_ref = fused.kv_append(q, k, v, rot, cos, sin, gq, gk, dc.APPEND_EPS, kr, vr)
    q_out = fused.kv_append_suffix(q, k, v, rot if tables else None, wr, cos, sin, gq, gk, dc.APPEND_EPS, kc, vc)
    rows = torch.arange(dc.APPEND_B, device=cuda)
    nm.assert_bits(q_out, q_ref, "q")
    nm.assert_bits(kc[rows, wr.long()], kr[rows, rot.long()], "appended k")
    nm.assert_bits(vc[rows, wr.long()], v.contiguous(), "appended v")

    def untouched(but):
        for cache, buf in ((kc, kbuf), (vc, vbuf)):
            rest = torch.ones(cache.shape[:2], dtype=torch.bool, device=cuda)
            rest[but, wr.long()[but]] = False
            assert bool((cache[rest] == dc.POISON).all()), "the cache is written outside cache[r, write_pos[r]]"
            assert bool((buf[:dc.GUARD] == dc.POISON).all()) and bool((buf[-dc.GUARD:] == dc.POISON).all()), "guard band"

    untouched(rows)
    fused.check_index_errors(blocking=True)
    # write positions outside [0, Ts): the flag is raised and those rows write nothing (row 3 writes as before)
    bad = torch.tensor([-1, dc.APPEND_TMAX, dc.APPEND_TMAX + 100000, WRITE[3]], dtype=torch.int32, device=cuda)
    fused.kv_append_suffix(q, k, v, rot if tables else None, bad, cos, sin, gq, gk, dc.APPEND_EPS, kc, vc)
    with pytest.raises(ValueError, match="KV cache"):
        fused.check_index_errors(blocking=True)
    untouched(rows)
