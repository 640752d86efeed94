"""gfx950 flash attention with per-row key bounds (document-isolated packing):
every document of a packed row against the fp64 reference of that document
run alone (tests/numerics.py), at head_dim 128 without dropout."""
import tempfile

import pytest
import torch

import numerics as nm
from distributed_lion_pytorch_amd.ops import fused, hip

D = 128
# (T, window, documents of batch row 0, of batch row 1): each batch row has its
# own layout, so the arrays' batch index is exercised
LAYOUTS = [
    (33, 0, [32, 1], [1, 32]),                    # one-token documents in the tail tile and at row 0
    (100, 0, [1, 31, 32, 33, 3], [100]),          # boundaries at 1, 32, 64, 97: mid-tile, aligned, shorter than a tile
    (257, 0, [70, 58, 128, 1], [129, 128]),       # a boundary on the 4-tile block (128); one token alone in the tail tile
    (1000, 0, [400, 350, 250], [1000]),           # whole blocks of skipped tiles beside an unsegmented row
    (300, 64, [150, 150], [40, 260]),             # the window folded into the bounds, shorter / longer than a document
]
HEADS = [(4, 2), (2, 2), (2, 1)]  # GQA on the LDS dK/dV kernel; H == Hkv (K in registers); a group of 2 on one kv head


def _spans(docs):
    out, s = [], 0
    for n in docs:
        out.append((s, s + n))
        s += n
    return out


def _position_ids(layout, device):
    return torch.stack([torch.cat([torch.arange(n, device=device) for n in docs]) for docs in layout])


def _inputs(B, T, H, Hkv, device, seed):
    g = torch.Generator().manual_seed(seed)  # drawn on the host: the same inputs on every device
    mk = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(device)  # noqa: E731
    return mk(B, T, H, D), mk(B, T, Hkv, D), mk(B, T, Hkv, D), mk(B, T, H * D)


def _run(q, k, v, dout, bounds):
    B, T, H, _ = q.shape
    assert fused._attn_ok(q, T, D, 0, bounds, 0.0)
    qs, ks, vs = (t.clone().requires_grad_() for t in (q, k, v))
    out = fused._FlashAttn.apply(qs, ks, vs, 0.0, 0, 0, bounds).view(B, T, H * D)
    out.backward(dout)
    return out, qs.grad, ks.grad, vs.grad


def _per_document_reference(q, k, v, dout, layout, window):
    """(ref, model, floor_q, floor_k): attention_ref64 of every document alone,
    plain and with the rounding model, scattered into full tensors; the zero
    floors per document (its first query has dq = 0, a one-token document
    dq = dk = 0)."""
    B, T = q.shape[:2]
    shapes = (dout.shape, q.shape, k.shape, v.shape)
    ref = [torch.zeros(s, dtype=torch.float64, device=q.device) for s in shapes]
    mod = [torch.zeros(s, dtype=torch.float64, device=q.device) for s in shapes]
    fq = torch.zeros(B, T, dtype=torch.float64, device=q.device)
    fk = torch.zeros(B, T, dtype=torch.float64, device=q.device)
    for b, docs in enumerate(layout):
        for s, e in _spans(docs):
            w = 0 if window >= e - s else window
            sl = [t[b:b + 1, s:e] for t in (q, k, v, dout)]
            r = nm.attention_ref64(*sl, 0.0, 0, w)
            m = nm.attention_ref64(*sl, 0.0, 0, w, model=True)
            for full, part in zip(ref + mod, r + m):
                full[b:b + 1, s:e] = part
            a, c = nm.attention_floors(r[1], r[3], e - s, w)
            fq[b:b + 1, s:e] = a
            if c is not None:
                fk[b:b + 1, s:e] = c
    return ref, mod, fq, fk


def _foreign_visible(docs, T):
    """Per row of one batch row, the number of foreign tokens on its visible
    side under plain causal attention: for a query (out, dQ) the keys before its
    own document, its start; for a key (dK, dV) the queries after its own
    document, T minus its end."""
    before, after = torch.zeros(T, dtype=torch.int64), torch.zeros(T, dtype=torch.int64)
    for s, e in _spans(docs):
        before[s:e] = s
        after[s:e] = T - e
    return before, after


def _assert_a_leak_could_not_pass(q, k, v, dout, layout, ref, mod, floors, tag):
    """The plain-causal rounding model of the whole row, put through the
    comparison that judges the kernels, exceeds C_ROWS on every row with a
    foreign document on its visible side (out, dQ: the rows after the first
    document; dK, dV: the rows before the last one).  References alone, no
    kernel.

    One exemption, by row and by count, not by layout: a row that a foreign
    document can reach through exactly ONE token.  For a query that is one
    foreign key before its document.  For a key it is one foreign query after
    its document while its own document's queries see at most one foreign key
    (a key's gradient also moves when its own queries' softmax is shared with
    earlier documents, so a key behind two or more foreign tokens is asserted
    whatever follows it).  Such a leak is a single term among the n of the row's
    sum, a share of about 1 / n, while the bound is C_ROWS x max(model error,
    2^-9 row max) -- about 8 x 2^-9 = 1.6 % of the row.  From n of a few tens on
    the two are of one size and the ratio falls on either side of C_ROWS with
    the draw (smallest on the CPU with these inputs: 0.0 for dQ at T = 100,
    1.2 for dK at T = 33), so no comparison at this bound separates such a row;
    their figures are printed.  Every other row is asserted, in every layout
    and head shape (smallest ratio on the CPU: 14.4)."""
    T = q.shape[1]
    leak = nm.attention_ref64(q, k, v, dout, 0.0, 0, 0, model=True)
    for b, docs in enumerate(layout):
        if len(docs) < 2:
            continue
        before, after = (t.to(q.device) for t in _foreign_visible(docs, T))
        for x, r, m, f, n in zip(leak, ref, mod, floors, ("out", "dq", "dk", "dv")):
            if n in ("out", "dq"):
                judged, single = before >= 2, before == 1
            else:
                judged, single = (after >= 2) | ((after == 1) & (before >= 2)), (after == 1) & (before <= 1)
            ratio = nm.rows_ratio(x.reshape(2, T, -1), r, m, f)[b]
            judged, single = ratio[judged], ratio[single]
            if single.numel():
                print(f"[leak] {tag} row {b} {n}: {single.numel()} rows with one foreign token, not asserted: "
                      f"ratio {float(single.min()):.1f} .. {float(single.max()):.1f}")
            if judged.numel():
                print(f"[leak] {tag} row {b} {n}: {judged.numel()} rows, min ratio {float(judged.min()):.1f}")
                assert float(judged.min()) > nm.C_ROWS, (tag, n, b, float(judged.min()))


@pytest.mark.gpu
@pytest.mark.parametrize("H,Hkv", HEADS, ids=[f"h{h}kv{g}" for h, g in HEADS])
@pytest.mark.parametrize("T,window,docs0,docs1", LAYOUTS, ids=[f"T{l[0]}w{l[1]}" for l in LAYOUTS])
def test_bounds_attention_matches_documents_run_alone(T, window, docs0, docs1, H, Hkv, cuda):
    """out, dQ, dK, dV of every row within C_ROWS x the rounding model of its
    own document's fp64 reference -- and that comparison could not pass a leak
    (_assert_a_leak_could_not_pass)."""
    hip.require()
    layout = (docs0, docs1)
    assert sum(docs0) == sum(docs1) == T
    q, k, v, dout = _inputs(2, T, H, Hkv, cuda, 1000 * T + 10 * H + Hkv)
    bounds = fused.visibility_bounds(_position_ids(layout, cuda), window)
    got = _run(q, k, v, dout, bounds)
    ref, mod, fq, fk = _per_document_reference(q, k, v, dout, layout, window)
    floors = (None, fq, fk, None)
    names = ("out", "dq", "dk", "dv")
    tag = f"T={T} w={window} H={H}/{Hkv}"
    _assert_a_leak_could_not_pass(q, k, v, dout, layout, ref, mod, floors, tag)

    failures = []
    for x, r, m, f, n in zip(got, ref, mod, floors, names):
        try:
            nm.assert_rows_close(x.reshape(2, T, -1), r, m, nm.C_ROWS, f, f"bounds {tag} {n}")
        except AssertionError as err:
            failures.append(str(err))
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
def test_a_document_is_bit_exactly_independent_of_its_neighbours(cuda):
    """T = 256, documents [64, 96, 96] (32-aligned: a wave's tile belongs to one
    document): replacing documents 0 and 2 leaves every bit of document 1's out,
    dQ, dK and dV -- masked probabilities are exact zeros, skipped tiles depend
    only on the bounds, and no foreign row takes part in a wave-wide vote."""
    hip.require()
    B, T, H, Hkv = 2, 256, 4, 2
    layout = ([64, 96, 96], [64, 96, 96])
    bounds = fused.visibility_bounds(_position_ids(layout, cuda))
    a = _inputs(B, T, H, Hkv, cuda, 11)
    other = _inputs(B, T, H, Hkv, cuda, 12)
    b = [t.clone() for t in a]
    for t, o in zip(b, other):
        t[:, :64] = o[:, :64]
        t[:, 160:] = o[:, 160:]
    ra, rb = _run(*a, bounds), _run(*b, bounds)
    for x, y, n in zip(ra, rb, ("out", "dq", "dk", "dv")):
        assert torch.equal(x[:, 64:160], y[:, 64:160]), n
        assert not torch.equal(x[:, :64], y[:, :64]), n  # the other documents did change


def _close(a, b, tol, floor=0.0):
    err = (a.float() - b.float()).abs().max().item()
    scale = max(b.float().abs().max().item(), floor) + 1e-6
    assert err <= tol * scale, f"max err {err} vs scale {scale}"


@pytest.mark.gpu
@pytest.mark.parametrize("head_dim,p", [(64, 0.0), (128, 0.1)])
def test_bounds_outside_the_flash_kernels_take_math_sdpa(head_dim, p, cuda, monkeypatch):
    """Bounds at head_dim 64, or with attention dropout, have no flash
    instantiation: one call of _sdpa_math, handed the bounds.  Its result against
    the fp32 reference of every document alone.  (ATen's math SDPA draws its own
    dropout mask, which no reference reproduces: the counting wrapper records the
    requested p and evaluates the call it was handed at p = 0, so what is compared
    is the mask built from the bounds.)"""
    import warnings

    hip.require()
    B, T, H, Hkv = 2, 100, 4, 2
    layout = ([1, 31, 32, 33, 3], [60, 40])
    torch.manual_seed(5)
    q = torch.randn(B, T, H, head_dim, device=cuda, dtype=torch.bfloat16)
    k = torch.randn(B, T, Hkv, head_dim, device=cuda, dtype=torch.bfloat16)
    v = torch.randn(B, T, Hkv, head_dim, device=cuda, dtype=torch.bfloat16)
    dout = torch.randn(B, T, H * head_dim, device=cuda, dtype=torch.bfloat16)
    bounds = fused.visibility_bounds(_position_ids(layout, cuda))
    assert not fused._attn_ok(q, T, head_dim, 0, bounds, p)
    calls = []
    real = fused._sdpa_math

    def counting(qh, kh, vh, dropout_p, window=0, bounds=None):
        calls.append((dropout_p, window, bounds))
        return real(qh, kh, vh, 0.0, window, bounds)

    monkeypatch.setattr(fused, "_sdpa_math", counting)
    qs, ks, vs = (t.clone().requires_grad_() for t in (q, k, v))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the fallback's one-time warning
        out = fused.causal_attention_gqa(qs, ks, vs, p, 0, bounds)
    out.backward(dout)
    assert len(calls) == 1 and calls[0][0] == p and calls[0][1] == 0 and calls[0][2] is not None
    refs = [torch.zeros(t.shape, device=cuda) for t in (dout, q, k, v)]
    for b, docs in enumerate(layout):
        for s, e in _spans(docs):
            qr, kr, vr = (t[b:b + 1, s:e].float().requires_grad_() for t in (q, k, v))
            r = fused.reference_attention(qr, kr, vr)
            r.backward(dout[b:b + 1, s:e].float())
            for full, part in zip(refs, (r.detach(), qr.grad, kr.grad, vr.grad)):
                full[b:b + 1, s:e] = part
    _close(out, refs[0], 2e-2)
    _close(qs.grad, refs[1], 3e-2)
    _close(ks.grad, refs[2], 3e-2)
    _close(vs.grad, refs[3], 3e-2)
    if p > 0:
        # the call as it stands, with ATen's own dropout mask: no reference for the
        # values, but the bounds-with-dropout branch runs forward and backward
        monkeypatch.setattr(fused, "_sdpa_math", real)
        qd, kd, vd = (t.clone().requires_grad_() for t in (q, k, v))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            dropped = fused.causal_attention_gqa(qd, kd, vd, p, 0, bounds)
        dropped.backward(dout)
        assert dropped.shape == out.shape and not torch.equal(dropped, out)
        for t in (dropped, qd.grad, kd.grad, vd.grad):
            assert torch.isfinite(t).all()
        assert qd.grad.shape == q.shape and kd.grad.shape == k.shape and vd.grad.shape == v.shape
    # reference_attention's own bounds argument is the same mask
    _close(fused.reference_attention(q.float(), k.float(), v.float(), bounds=bounds), refs[0], 1e-5)


@pytest.mark.gpu
def test_llama_with_position_ids_matches_hf_per_document(cuda, monkeypatch):
    """A 2-layer Llama (head_dim 128, 2 heads on 1 kv head) in bf16 with
    position_ids for documents [90, 130, 80] against HF's model in fp32 run on
    each document alone: token-weighted loss, summed gradients; again with
    gradient checkpointing.  The flash kernels run, not the math fallback."""
    import transformers

    from distributed_lion_pytorch_amd.models.llama import LlamaForCausalLM

    hip.require()
    torch.manual_seed(3)
    cfg = transformers.LlamaConfig(vocab_size=256, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                                   num_attention_heads=2, num_key_value_heads=1, max_position_embeddings=512)
    ours = LlamaForCausalLM(cfg)
    with tempfile.TemporaryDirectory() as d:
        ours.save_pretrained(d)
        hf = transformers.LlamaForCausalLM.from_pretrained(d)
    ours, hf = ours.to(cuda, torch.bfloat16), hf.to(cuda, torch.float32)
    docs, B, T = [90, 130, 80], 2, 300
    ids = torch.randint(0, 256, (B, T), device=cuda)
    pos = _position_ids((docs, docs), cuda)
    labels = ids.clone()
    labels[pos == 0] = -100
    total, count = 0.0, 0
    for b in range(B):
        for s, e in _spans(docs):
            x = ids[b:b + 1, s:e]
            total = total + hf(x, labels=x).loss * (e - s - 1)
            count += e - s - 1
    lb = total / count
    lb.backward()
    math_calls = []
    real = fused._sdpa_math
    monkeypatch.setattr(fused, "_sdpa_math", lambda *a, **kw: (math_calls.append(1), real(*a, **kw))[1])
    ours.train()
    for checkpointing in (False, True):
        if checkpointing:
            ours.gradient_checkpointing_enable()
        ours.zero_grad(set_to_none=True)
        la = ours(ids, labels=labels, position_ids=pos).loss
        assert abs(la.item() - lb.item()) < 2e-2, (checkpointing, la.item(), lb.item())
        la.backward()
        for (n, p_), (_, r) in zip(ours.named_parameters(), hf.named_parameters()):
            if r.grad is not None and r.grad.abs().max() > 0:
                err = (p_.grad.float() - r.grad).abs().max().item() / r.grad.abs().max().item()
                assert err < 0.1, (checkpointing, n, err)
    assert not math_calls
    fused.check_index_errors(blocking=True)  # the position_ids were valid


@pytest.mark.gpu
def test_cuda_position_ids_that_jump_raise_through_the_index_flag(cuda):
    """On the GPU a jump inside a document is reported by the per-step index
    flag (no host sync in visibility_bounds), like an out-of-range token id.
    The arrays built from such input are not handed to a kernel here."""
    fused.check_index_errors(blocking=True)  # start clean
    pos = torch.cat([torch.arange(5), torch.arange(7)])[None].to(cuda)
    fused.visibility_bounds(pos)
    fused.check_index_errors(blocking=True)
    pos[0, 8] = 9
    fused.visibility_bounds(pos)  # does not raise here
    with pytest.raises(ValueError, match="position_ids"):
        fused.check_index_errors(blocking=True)
    fused.check_index_errors(blocking=True)  # the flag was cleared
