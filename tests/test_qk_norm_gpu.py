"""The per-head q/k RMSNorm + RoPE kernels (csrc/qk_norm.hip) and the native
Qwen3 path on the GPU.  The kernels are judged against the fp64 form of
fused.qk_norm_rope_reference: one bf16 rounding plus a per-head-row floor that
comes from the reference's own fp32 evaluation (tests/qk_norm_cases.py,
docs/TEST_TOLERANCES.md "q/k norm"), never from what the kernels give."""
import functools
import tempfile

import pytest
import torch
import transformers

import numerics as nm
import qk_norm_cases as qc
from distributed_lion_pytorch_amd.models import llama as L
from distributed_lion_pytorch_amd.ops import fused, hip
from distributed_lion_pytorch_amd.ops import linear as lin

pytestmark = pytest.mark.gpu
B = qc.B
# token rows B T -> parts: more parts than rows at T = 1, a ragged last part at the others
PARTS = {1: 5, 33: 7, 100: 9}


@functools.lru_cache(maxsize=None)
def _case(T, H, Hkv, D):
    """Inputs and the fp64 / fp32 forms of one shape, computed once on the host and shared by the tests."""
    x, dz, gq, gk, cos, sin = qc.inputs(T, H, Hkv, D)
    c = dict(x=x, dz=dz, gq=gq, gk=gk, cos=cos, sin=sin)
    z64, dx64, dgq64, dgk64 = qc.form(x, gq, gk, H, cos, sin, dz, torch.float64)
    z32, dx32, _, _ = qc.form(x, gq, gk, H, cos, sin, dz, torch.float32)
    c.update(z64=z64, floor_z=qc.row_floor(z32, z64), dx64=dx64, floor_dx=qc.row_floor(dx32, dx64), dgq64=dgq64,
             dgk64=dgk64, rstd64=qc.stats64(x)[1])
    # the second backward mode: dy = bf16(rope^T(dz)) handed over without tables
    dy = nm._rope64_bwd(dz.double(), cos, sin).to(torch.bfloat16)
    _, dxy64, dgqy64, dgky64 = qc.form(x, gq, gk, H, cos, sin, dy, torch.float64, rotate=False)
    _, dxy32, _, _ = qc.form(x, gq, gk, H, cos, sin, dy, torch.float32, rotate=False)
    c.update(dy=dy, dxy64=dxy64, floor_dxy=qc.row_floor(dxy32, dxy64), dgqy64=dgqy64, dgky64=dgky64)
    return c


def _layouts(t, Hkv, device, fill=0.0):
    """t [B, T, Hx, D] on the device, contiguous, and as the q | k column view of a [B, T, (Hx + Hkv) D] buffer
    whose v columns hold ``fill``; yields (name, view, buffer or None)."""
    Bn, T, Hx, D = t.shape
    yield "contiguous", t.to(device).contiguous(), None
    buf = torch.full((Bn, T, (Hx + Hkv) * D), fill, dtype=t.dtype, device=device)
    view = buf[..., :Hx * D].view(Bn, T, Hx, D)
    view.copy_(t)
    yield "q|k view", view, buf


def _dev(c, device, *names):
    return tuple(c[n].to(device) for n in names)


@pytest.mark.parametrize("T,H,Hkv,D", qc.SHAPES)
def test_forward(T, H, Hkv, D, cuda):
    hip.require()
    c = _case(T, H, Hkv, D)
    gq, gk, cos, sin = _dev(c, cuda, "gq", "gk", "cos", "sin")
    for name, x, _ in _layouts(c["x"], Hkv, cuda):
        y, rstd = hip.ops().qk_norm_rope_fwd(x, gq, gk, H, qc.EPS, cos, sin)
        tag = f"fwd T={T} H={H}/{Hkv} D={D} {name}"
        assert y.shape == x.shape and y.is_contiguous() and y.dtype == torch.bfloat16
        assert rstd.shape == (B, T, H + Hkv) and rstd.dtype == torch.float32
        nm.assert_rounded(y.cpu(), c["z64"], c["floor_z"], tag)
        ratio = float(((rstd.cpu().double() - c["rstd64"]).abs() / (4 * 2.0 ** -24 * c["rstd64"])).max())
        print(f"[rstd] {tag}: max err / (4 x 2^-24 |ref|) {ratio:.3f}")
        assert ratio <= 1.0, tag
        assert bool((y[0, 0, 0] == 0).all()) and float(rstd[0, 0, 0]) == pytest.approx(1e3, rel=1e-6)


@pytest.mark.parametrize("mode", ["dz+tables", "dy"])
@pytest.mark.parametrize("T,H,Hkv,D", qc.SHAPES)
def test_backward(T, H, Hkv, D, mode, cuda):
    """dx in place and the gain-gradient partials, with dz plus tables and with a pre-rotated bf16 dy and none,
    each against the fp64 form of its own input; the partial stack summed by sum_partials gives the gain
    gradients (the tolerance of the norm-gain tests, on the mean magnitude)."""
    hip.require()
    c = _case(T, H, Hkv, D)
    gq, gk, cos, sin = _dev(c, cuda, "gq", "gk", "cos", "sin")
    rot = mode == "dz+tables"
    g_in, dx64, floor = (c["dz"], c["dx64"], c["floor_dx"]) if rot else (c["dy"], c["dxy64"], c["floor_dxy"])
    dg64 = torch.stack([c["dgq64"], c["dgk64"]] if rot else [c["dgqy64"], c["dgky64"]])
    parts = PARTS[T]
    for (name, x, _), (_, g, gbuf) in zip(_layouts(c["x"], Hkv, cuda), _layouts(g_in, Hkv, cuda, fill=3.0)):
        tag = f"bwd {mode} T={T} H={H}/{Hkv} D={D} {name}"
        _, rstd = hip.ops().qk_norm_rope_fwd(x, gq, gk, H, qc.EPS, cos, sin)
        part = hip.ops().qk_norm_rope_bwd_(g, x, rstd, gq, gk, H, cos if rot else None, sin if rot else None, parts)
        nm.assert_rounded(g.cpu(), dx64, floor, tag + " dx")
        if gbuf is not None:  # the dv columns of the packed gradient buffer are not the op's
            assert bool((gbuf[..., (H + Hkv) * D:] == 3.0).all()), tag
        qc.assert_gain_partials(part, c["x"], g_in, c["cos"], c["sin"], H, parts, c["floor_z"], rot, tag)
        sums = hip.ops().sum_partials(part)
        assert sums.shape == (2, D) and sums.dtype == torch.bfloat16
        for i, n in enumerate(("q", "k")):
            nm.assert_elems_close(sums[i].cpu(), dg64[i], 2e-2, nm.vec_atol(dg64[i], 2e-2), f"{tag} d gamma_{n}")


@pytest.mark.parametrize("T,H,Hkv,D", [(33, 4, 2, 128), (100, 3, 1, 64), (1, 2, 2, 128)])
def test_deterministic_and_one_launch_equals_two(T, H, Hkv, D, cuda):
    hip.require()
    c = _case(T, H, Hkv, D)
    gq, gk, cos, sin = _dev(c, cuda, "gq", "gk", "cos", "sin")
    ops, parts = hip.ops(), PARTS[T]
    _, x, _ = list(_layouts(c["x"], Hkv, cuda))[1]

    def run(rot):
        y, rstd = ops.qk_norm_rope_fwd(x, gq, gk, H, qc.EPS, cos, sin)
        _, g, _ = list(_layouts(c["dz"], Hkv, cuda))[1]
        part = ops.qk_norm_rope_bwd_(g, x, rstd, gq, gk, H, cos if rot else None, sin if rot else None, parts)
        return y, rstd, g.clone(), part

    for rot in (True, False):
        a, b = run(rot), run(rot)
        for u, v, n in zip(a, b, ("y", "rstd", "dx", "part")):
            nm.assert_bits(u, v, f"two runs, {n}")
        # q and k in two launches of their own (gamma_b absent: split == the head count)
        xq, xk = x[:, :, :H], x[:, :, H:]
        yq, rq = ops.qk_norm_rope_fwd(xq, gq, None, H, qc.EPS, cos, sin)
        yk, rk = ops.qk_norm_rope_fwd(xk, gk, None, Hkv, qc.EPS, cos, sin)
        nm.assert_bits(torch.cat([yq, yk], 2), a[0], "one launch against two, y")
        nm.assert_bits(torch.cat([rq, rk], 2), a[1], "one launch against two, rstd")
        _, g, _ = list(_layouts(c["dz"], Hkv, cuda))[1]
        t = (cos, sin) if rot else (None, None)
        pq = ops.qk_norm_rope_bwd_(g[:, :, :H], xq, rq, gq, None, H, *t, parts)
        pk = ops.qk_norm_rope_bwd_(g[:, :, H:], xk, rk, gk, None, Hkv, *t, parts)
        nm.assert_bits(g, a[2], "one launch against two, dx")
        nm.assert_bits(torch.stack([pq[:, 0], pk[:, 0]], 1), a[3], "one launch against two, partials")
        assert bool((pq[:, 1] == 0).all()) and bool((pk[:, 1] == 0).all())


def test_op_checks(cuda):
    hip.require()
    c = _case(33, 2, 2, 64)
    x, gq, gk, cos, sin = _dev(c, cuda, "x", "gq", "gk", "cos", "sin")
    ops = hip.ops()
    with pytest.raises(RuntimeError, match="head_dim must be 64 or 128"):
        ops.qk_norm_rope_fwd(x[..., :32].contiguous(), gq[:32].contiguous(), None, 4, qc.EPS, cos[:, :32].contiguous(),
                             sin[:, :32].contiguous())
    with pytest.raises(RuntimeError, match="split"):
        ops.qk_norm_rope_fwd(x, gq, None, 2, qc.EPS, cos, sin)
    with pytest.raises(RuntimeError, match="cos/sin"):
        ops.qk_norm_rope_fwd(x, gq, gk, 2, qc.EPS, cos[:10].contiguous(), sin[:10].contiguous())
    with pytest.raises(RuntimeError, match="contiguous heads"):
        ops.qk_norm_rope_fwd(x.transpose(1, 2).contiguous().transpose(1, 2), gq, gk, 2, qc.EPS, cos, sin)
    y, rstd = ops.qk_norm_rope_fwd(x, gq, gk, 2, qc.EPS, cos, sin)
    with pytest.raises(RuntimeError, match="pair"):
        ops.qk_norm_rope_bwd_(y, x, rstd, gq, gk, 2, cos, None, 4)
    with pytest.raises(RuntimeError, match="parts"):
        ops.qk_norm_rope_bwd_(y, x, rstd, gq, gk, 2, None, None, 0)


# ------------------------------------------------------------------ autograd wiring
def _norm64(x, gamma):
    x64 = x.detach().double()
    return gamma.detach().double() * (x64 * torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + qc.EPS))


def _norm64_bwd(x, gamma, dyn):
    """(dx, dgamma) of _norm64 for the output gradient dyn, by autograd in fp64."""
    x64, g64 = x.detach().double().requires_grad_(), gamma.detach().double().requires_grad_()
    y = g64 * (x64 * torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + qc.EPS))
    y.backward(dyn.double())
    return x64.grad, g64.grad


def _attn_inputs(device, T=100, H=4, Hkv=2, D=128, seed=0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, generator=g).to(torch.bfloat16).to(device)
    dout = torch.randn(B, T, H * D, generator=g).to(torch.bfloat16).to(device)
    gq = (1 + 0.25 * torch.randn(D, generator=g)).to(torch.bfloat16).to(device)
    gk = (1 + 0.25 * torch.randn(D, generator=g)).to(torch.bfloat16).to(device)
    cos, sin = L.Rotary(D, 10000.0).tables(T, device, torch.bfloat16)
    return qkv, dout, gq, gk, cos, sin


def _split(qkv, H, Hkv, D):
    Bn, T, _ = qkv.shape
    q = qkv[..., :H * D].view(Bn, T, H, D)
    k = qkv[..., H * D:(H + Hkv) * D].view(Bn, T, Hkv, D)
    v = qkv[..., (H + Hkv) * D:].view(Bn, T, Hkv, D)
    return q, k, v


@pytest.mark.parametrize("adjacent", [True, False])
@pytest.mark.parametrize("rope_bwd_fused", [True, False])
def test_rope_attention_with_gains(rope_bwd_fused, adjacent, cuda, monkeypatch):
    """rope_attention(..., q_gamma, k_gamma) at T = 100, 4 / 2 heads, D = 128 against attention_ref64 fed the fp64
    normed q / k: out, dq, dk, dv row by row at C_ROWS, dq / dk of the reference and of the rounding model carried
    through the fp64 norm backward; with the inverse rotation in the attention kernels' stores and as the norm
    backward's first step; on the q | k | v views of one buffer (one launch) and on separate tensors (two)."""
    hip.require()
    T, H, Hkv, D = 100, 4, 2, 128
    monkeypatch.setattr(fused, "_ROPE_BWD_FUSED", rope_bwd_fused)
    monkeypatch.setattr(fused, "_sdpa_math", lambda *a, **kw: pytest.fail("math SDPA fallback"))
    qkv, dout, gq, gk, cos, sin = _attn_inputs(cuda)
    gq.requires_grad_()
    gk.requires_grad_()
    if adjacent:
        leaf = qkv.clone().requires_grad_()
        q, k, v = _split(leaf, H, Hkv, D)
        assert fused._adjacent_heads(q, k) is not None
    else:
        leaves = [t.clone().requires_grad_() for t in _split(qkv, H, Hkv, D)]
        q, k, v = leaves
        assert fused._adjacent_heads(q, k) is None
    out = fused.rope_attention(q, k, v, cos, sin, q_gamma=gq, k_gamma=gk, eps=qc.EPS)
    out.backward(dout)
    if adjacent:
        dq, dk, dv = _split(leaf.grad, H, Hkv, D)
    else:
        dq, dk, dv = (t.grad for t in leaves)
    q0, k0, v0 = _split(qkv, H, Hkv, D)
    qn, kn = _norm64(q0, gq), _norm64(k0, gk)
    ref = nm.attention_ref64(qn, kn, v0, dout, 0.0, 0, 0, cos, sin)
    mod = nm.attention_ref64(qn, kn, v0, dout, 0.0, 0, 0, cos, sin, model=True)
    (rdq, rgq), (rdk, rgk) = _norm64_bwd(q0, gq, ref[1]), _norm64_bwd(k0, gk, ref[2])
    (mdq, _), (mdk, _) = _norm64_bwd(q0, gq, mod[1]), _norm64_bwd(k0, gk, mod[2])
    fq, fk = nm.attention_floors(rdq, ref[3], T)
    tag = f"qk-norm attention rot-in-attn={rope_bwd_fused} adjacent={adjacent}"
    failures = []
    for g_, r, m, f, n in ((out, ref[0], mod[0], None, "out"), (dq, rdq, mdq, fq, "dq"), (dk, rdk, mdk, fk, "dk"),
                           (dv, ref[3], mod[3], None, "dv")):
        try:
            nm.assert_rows_close(g_.reshape(B, T, -1), r.reshape(B, T, -1), m.reshape(B, T, -1), nm.C_ROWS, f,
                                 f"{tag} {n}")
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
    for got, r, n in ((gq.grad, rgq, "q_gamma"), (gk.grad, rgk, "k_gamma")):
        assert got.dtype == torch.bfloat16 and got.shape == (D,)
        nm.assert_elems_close(got, r, 2e-2, nm.vec_atol(r, 2e-2), f"{tag} d {n}")


def test_rope_attention_without_gains_is_unchanged(cuda, monkeypatch):
    """q_gamma = None: the autograd function that ran before runs, bit for bit."""
    hip.require()
    T, H, Hkv, D = 100, 4, 2, 128
    qkv, dout, _, _, cos, sin = _attn_inputs(cuda, seed=1)
    monkeypatch.setattr(fused._QKNormRopeAttention, "forward", lambda *a, **kw: pytest.fail("the q/k norm path ran"))
    a, b = qkv.clone().requires_grad_(), qkv.clone().requires_grad_()
    out = fused.rope_attention(*_split(a, H, Hkv, D), cos, sin)
    out.backward(dout)
    old = fused._RopeAttention.apply(*_split(b, H, Hkv, D), cos, sin, 0.0, 0, 0, None).view(B, T, H * D)
    old.backward(dout)
    nm.assert_bits(out, old, "out")
    nm.assert_bits(a.grad, b.grad, "dq | dk | dv")


def test_gain_gradients_in_the_fusion_window(cuda):
    """Two micro-batches inside grad_accumulation_fusion: q_norm / k_norm gains take the deposit path of the other
    RMSNorm gains, and their .grad is the sum of the two separately computed gradients to within one bf16 ulp of
    the largest of the two and their sum."""
    hip.require()
    T, H, Hkv, D = 100, 4, 2, 128
    batches = [_attn_inputs(cuda, seed=s) for s in (2, 3)]
    _, _, gq0, gk0, cos, sin = batches[0]
    gq, gk = torch.nn.Parameter(gq0.clone()), torch.nn.Parameter(gk0.clone())

    def step(qkv, dout):
        leaf = qkv.clone().requires_grad_()
        fused.rope_attention(*_split(leaf, H, Hkv, D), cos, sin, q_gamma=gq, k_gamma=gk, eps=qc.EPS).backward(dout)

    single = []
    for qkv, dout, *_ in batches:
        gq.grad = gk.grad = None
        step(qkv, dout)
        single.append((gq.grad.clone(), gk.grad.clone()))
    gq.grad = gk.grad = None
    with lin.grad_accumulation_fusion(True, micro_batches=2):
        for qkv, dout, *_ in batches:
            step(qkv, dout)
    for i, (p, n) in enumerate(((gq, "q_norm"), (gk, "k_norm"))):
        a, b = single[0][i].double(), single[1][i].double()
        assert p.grad is not None and p.grad.dtype == torch.bfloat16
        ulp = 2 * nm.bf16_half_ulp(torch.maximum(torch.maximum(a.abs(), b.abs()), (a + b).abs()))
        err = (p.grad.double() - (a + b)).abs()
        print(f"[window] {n}.weight.grad: max err / ulp {float((err / ulp).max()):.3f}")
        assert bool((err <= ulp).all()), n


# ------------------------------------------------------------------------- model
def _qwen3_cfg(**kw):
    return transformers.Qwen3Config(vocab_size=256, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                                    num_attention_heads=2, num_key_value_heads=1, head_dim=128,
                                    max_position_embeddings=512, tie_word_embeddings=False, **kw)


def _spy_head_row_norms(monkeypatch, seen):
    """Record every torch rms_norm / pow over rows of head_dim (128) elements: the ATen RMSNorm chain on head rows."""
    def wrap(owner, name):
        real = getattr(owner, name)

        def spy(*a, **kw):
            t = a[0] if a else None
            if torch.is_tensor(t) and t.dim() >= 3 and t.shape[-1] == 128:
                seen.append((name, tuple(t.shape)))
            return real(*a, **kw)

        monkeypatch.setattr(owner, name, spy)

    wrap(torch, "rms_norm")
    wrap(torch.nn.functional, "rms_norm")
    wrap(torch, "pow")
    wrap(torch.Tensor, "pow")


def _pair(cuda):
    torch.manual_seed(3)
    ours = L.Qwen3ForCausalLM(_qwen3_cfg())
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for n, p in ours.named_parameters():
            if "q_norm" in n or "k_norm" in n:
                p.copy_(1.0 + 0.25 * torch.randn(p.shape, generator=g))
    with tempfile.TemporaryDirectory() as d:
        ours.save_pretrained(d)
        hf = transformers.Qwen3ForCausalLM.from_pretrained(d)
    return ours.to(cuda, torch.bfloat16), hf.to(cuda, torch.float32)


def test_qwen3_matches_hf_fp32(cuda, monkeypatch):
    """2-layer Qwen3 (hidden 256, 2 heads on 1 kv head, head_dim 128) in bf16 against HF in fp32: plain, with
    gradient checkpointing, and with position_ids for documents [90, 130, 80] against HF on each document alone.
    The flash kernels and the q/k norm op run: no math SDPA and no ATen norm chain over head rows."""
    hip.require()
    ours, hf = _pair(cuda)
    docs, T = [90, 130, 80], 300
    ids = torch.randint(0, 256, (B, T), device=cuda)
    pos = torch.stack([torch.cat([torch.arange(n, device=cuda) for n in docs])] * B)
    plabels = ids.clone()
    plabels[pos == 0] = -100

    lb = hf(ids, labels=ids).loss
    lb.backward()
    plain = (lb.item(), {n: p.grad.clone() for n, p in hf.named_parameters()})
    hf.zero_grad(set_to_none=True)
    total, count, s = 0.0, 0, 0
    for n in docs:
        for b in range(B):
            x = ids[b:b + 1, s:s + n]
            total = total + hf(x, labels=x).loss * (n - 1)
            count += n - 1
        s += n
    lp = total / count
    lp.backward()
    packed = (lp.item(), {n: p.grad.clone() for n, p in hf.named_parameters()})

    math_calls, chain, op_calls = [], [], []
    real = fused._sdpa_math
    monkeypatch.setattr(fused, "_sdpa_math", lambda *a, **kw: (math_calls.append(1), real(*a, **kw))[1])
    real_fwd = fused._QKNormRopeAttention.forward
    monkeypatch.setattr(fused._QKNormRopeAttention, "forward",
                        staticmethod(lambda *a, **kw: (op_calls.append(1), real_fwd(*a, **kw))[1]))
    _spy_head_row_norms(monkeypatch, chain)
    ours.train()
    for what, kw, (ref_loss, ref_grads) in (("plain", dict(labels=ids), plain),
                                            ("checkpointing", dict(labels=ids), plain),
                                            ("position_ids", dict(labels=plabels, position_ids=pos), packed)):
        if what == "checkpointing":
            ours.gradient_checkpointing_enable()
        else:
            ours.gradient_checkpointing_disable()
        ours.zero_grad(set_to_none=True)
        n_ops = len(op_calls)
        la = ours(ids, **kw).loss
        assert abs(la.item() - ref_loss) < 2e-2, (what, la.item(), ref_loss)
        la.backward()
        for n, p in ours.named_parameters():
            r = ref_grads[n]
            assert p.grad is not None, (what, n)
            if r.abs().max() > 0:
                err = (p.grad.float() - r).abs().max().item() / r.abs().max().item()
                assert err < 0.1, (what, n, err)
        assert len(op_calls) - n_ops >= 2, what  # one per layer (again in a checkpointed backward)
    assert not math_calls
    assert not chain, chain[:3]
    fused.check_index_errors(blocking=True)
    at = ours.model.layers[0].self_attn  # pack_projections: q | k | v weights share one buffer after the first step
    assert at.k_proj.weight.data_ptr() == at.q_proj.weight.data_ptr() + at.q_proj.weight.numel() * 2
    # sequence_logps (DPO) runs the same path
    n_ops = len(op_calls)
    with torch.no_grad():
        lps = ours.sequence_logps(ids, ids)
    ref = torch.log_softmax(hf(ids).logits[:, :-1].float(), -1).gather(-1, ids[:, 1:, None])[..., 0].sum(-1)
    assert len(op_calls) - n_ops == 2 and torch.allclose(lps.float(), ref, rtol=2e-2), (lps, ref)


def _spy_op(monkeypatch):
    calls = []
    real_fwd = fused._QKNormRopeAttention.forward
    monkeypatch.setattr(fused._QKNormRopeAttention, "forward",
                        staticmethod(lambda *a, **kw: (calls.append(1), real_fwd(*a, **kw))[1]))
    monkeypatch.setattr(fused, "_sdpa_math", lambda *a, **kw: pytest.fail("math SDPA fallback"))
    return calls


_TARGETS = ["q_proj", "k_proj", "v_proj", "o_proj"]


def test_qwen3_lora_merge(cuda, monkeypatch):
    """LoRA on q / k / v / o (the q and k adapters add to the projection before the head norm): the loss before
    and after merging the adapters into the bf16 base weights agrees."""
    from distributed_lion_pytorch_amd.models.lora import LoraConfig, inject_lora, merge_and_unload

    hip.require()
    ours, _ = _pair(cuda)
    op_calls = _spy_op(monkeypatch)
    inject_lora(ours, LoraConfig(r=8, lora_alpha=16, lora_dropout=0.0, target_modules=_TARGETS))
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for n, p in ours.named_parameters():
            if "lora_B" in n:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    ours.train()
    ids = torch.randint(0, 256, (B, 200), device=cuda)
    la = ours(ids, labels=ids).loss
    la.backward()
    assert len(op_calls) == 2
    for n, p in ours.named_parameters():
        if "lora_" in n:
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
    with torch.no_grad():
        lm = merge_and_unload(ours)(ids, labels=ids).loss
    assert abs(lm.item() - la.item()) < 2e-2, (la.item(), lm.item())  # the merged weight: one more bf16 rounding


def test_qwen3_qlora_matches_dequantized(cuda, monkeypatch):
    """Linear4bit bases under LoRA on q / k / v / o equal LoRA over the dequantised bf16 weights (the tolerances
    of test_qlora_llama_gpu_matches_dequantized)."""
    from distributed_lion_pytorch_amd.models.lora import LoraConfig, inject_lora
    from distributed_lion_pytorch_amd.models.quant import Linear4bit, QuantConfig, dequantize_model, quantize_model

    hip.require()
    qc4 = QuantConfig(bnb_4bit_compute_dtype=torch.bfloat16)
    m4 = quantize_model(_pair(cuda)[0], qc4)
    mr = dequantize_model(quantize_model(_pair(cuda)[0], qc4))
    assert isinstance(m4.model.layers[0].self_attn.q_proj, Linear4bit)
    op_calls = _spy_op(monkeypatch)
    lc = LoraConfig(r=8, lora_alpha=16, lora_dropout=0.0, target_modules=_TARGETS)
    inject_lora(m4, lc)
    inject_lora(mr, lc)
    byname = dict(mr.named_parameters())
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for n, p in m4.named_parameters():
            if "lora_" in n:
                if "lora_B" in n:
                    p.copy_(0.02 * torch.randn(p.shape, generator=g))
                byname[n].copy_(p)
    ids = torch.randint(0, 256, (B, 128), device=cuda)
    l4, lr = m4(input_ids=ids, labels=ids).loss, mr(input_ids=ids, labels=ids).loss
    assert abs(l4.item() - lr.item()) < 1e-2
    l4.backward()
    lr.backward()
    assert len(op_calls) == 4
    for n, p in m4.named_parameters():
        if p.requires_grad:
            gr = byname[n].grad.float()
            assert (p.grad.float() - gr).abs().max().item() <= 5e-2 * gr.abs().max().item() + 1e-6, n
