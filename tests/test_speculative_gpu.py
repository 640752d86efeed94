"""Speculative decoding on the GPU in bf16 with kernel-eligible tiny models (hidden 256, 2 layers; GPT-2 at head_dim
64, Llama at head_dim 128 with GQA 4:1, a Mistral window, Qwen3): the chunk path (csrc/chunk_attention.hip) against
the full forward, both judged on the same model in fp32; rollback (KVCache.truncate) leaves nothing stale;
generate(assistant_model=...) against plain greedy decoding wherever the fp32 twin's argmax is decided.
docs/TEST_TOLERANCES.md "Chunk attention / speculative decoding" has the conditions and the measured figures."""
import pytest
import torch
import transformers

from distributed_lion_pytorch_amd.models import KVCache
from distributed_lion_pytorch_amd.models import llama as L
from distributed_lion_pytorch_amd.models.gpt2 import GPT2LMHeadModel, gpt2_config
from distributed_lion_pytorch_amd.ops import fused, hip

pytestmark = pytest.mark.gpu

FAMILIES = ["gpt2", "llama", "mistral", "qwen3"]
SEQ, LENS, CHUNK = 96, (17, 64, 65), 5
# the condition of tests/test_generate_gpu.py::test_teacher_forced_consistency, for the reason given there: the chunk
# path's logit error may be this many times the full bf16 forward's at the same position
MAX_RATIO = 2.0
T0, NEW, MIN_PREFIX = 20, 24, 16
# (model seed, prompt seed, spread) per family: chosen so that plain greedy decoding alone has a decided prefix of at
# least MIN_PREFIX tokens in every row (test_plain_greedy_has_a_decided_prefix asserts it); spread is the standard
# deviation of the log of the LM head's row scales in the token comparisons (build).  A search over spreads 1.5, 2
# and 3, model seeds 0..7 and prompt seeds 11..14 (the PyTorch forms in bf16) found no decided run with more varied
# tokens than these: with random weights, positions whose argmax bf16 resolves are mostly repeats.
SEEDS = {"gpt2": (0, 13, 0.0), "llama": (2, 13, 3.0), "mistral": (2, 13, 3.0), "qwen3": (1, 13, 2.0)}


def _llama_kw(layers, **kw):
    return dict(vocab_size=256, hidden_size=256, intermediate_size=512, num_hidden_layers=layers, num_attention_heads=4,
                num_key_value_heads=1, head_dim=128, max_position_embeddings=512, tie_word_embeddings=False, **kw)


def build(family, seed=0, layers=2, spread=0.0):
    torch.manual_seed(seed)
    if family == "gpt2":
        m = GPT2LMHeadModel(gpt2_config("gpt2", n_embd=256, n_layer=layers, n_head=4, vocab_size=256, n_positions=256,
                                        resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0, bos_token_id=0, eos_token_id=0))
    elif family == "llama":
        m = L.LlamaForCausalLM(transformers.LlamaConfig(**_llama_kw(layers)))
    elif family == "mistral":
        m = L.MistralForCausalLM(transformers.MistralConfig(**_llama_kw(layers, sliding_window=32)))
    else:
        m = L.Qwen3ForCausalLM(transformers.Qwen3Config(**{**_llama_kw(layers), "num_key_value_heads": 2}))
        g = torch.Generator().manual_seed(4 + seed)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if "q_norm" in n or "k_norm" in n:
                    p.copy_(1.0 + 0.25 * torch.randn(p.shape, generator=g))
    if spread and family != "gpt2":
        # the token comparisons only: an untied random lm_head gives near-uniform logits whose top two are closer than
        # bf16 resolves at one position in five; log-normal row scales (the same draw for every model, so that drafts
        # are not hopeless) widen the margins without touching anything under test
        g = torch.Generator().manual_seed(1234)
        with torch.no_grad():
            m.lm_head.weight.mul_(torch.exp(spread * torch.randn(m.lm_head.weight.shape[0], 1, generator=g)))
    return m.eval()


_PAIRS = {}


def pair(family, device, seed=0, layers=2, spread=0.0):
    """(the model in bf16, the same weights in fp32), built once."""
    key = (family, seed, layers, spread, str(device))
    if key not in _PAIRS:
        m, ref = build(family, seed, layers, spread), build(family, seed, layers, spread)
        m = m.to(device, torch.bfloat16)
        ref.load_state_dict({k: v.float() for k, v in m.state_dict().items()})  # the bf16-rounded weights, in fp32
        _PAIRS[key] = (m, ref.to(device))
    return _PAIRS[key]


def target(family, device):
    return pair(family, device, SEEDS[family][0], 2, SEEDS[family][2])


def assistants(family, device):
    s, spread = SEEDS[family][0], SEEDS[family][2]
    return {"self": target(family, device)[0], "one layer": pair(family, device, s + 101, 1, spread)[0],
            "other seed": pair(family, device, s + 202, 2, spread)[0]}


def prompts(family, device):
    ids = torch.randint(1, 256, (3, T0), generator=torch.Generator().manual_seed(SEEDS[family][1])).to(device)
    mask = torch.ones_like(ids)
    mask[0, :7] = 0  # left-padded row
    return ids, mask


def kernels_only(monkeypatch):
    for name in ("decode_attention_reference", "kv_append_reference", "chunk_attention_reference",
                 "kv_append_chunk_reference"):
        monkeypatch.setattr(fused, name, lambda *a, _n=name, **kw: pytest.fail(f"PyTorch {_n} ran"))


def exact_logits(ref, seq):
    fused.set_impl("torch")
    try:
        with torch.no_grad():
            return ref(seq).logits.float()
    finally:
        fused.set_impl("auto")


def chunked_teacher_forced(m, seq, lens):
    """Logits of the chunk path at every (row, position) from lens[b] - 1 on: [B, SEQ, V] (NaN where not computed),
    the cache, and the hidden-to-logits closure.  The prefill takes max(LENS) columns, the rest comes in chunks of
    CHUNK tokens per row, ragged where a row runs out of tokens."""
    B, dev = seq.shape[0], seq.device
    W = max(LENS)
    steps = -(-(SEQ - min(LENS)) // CHUNK)
    rows = torch.arange(B, device=dev)
    cache = KVCache(m.config, B, W + steps * CHUNK, dev, m.lm_head.weight.dtype)
    out = torch.full((B, SEQ, m.config.vocab_size), float("nan"), device=dev)
    t = torch.arange(CHUNK, device=dev)
    with torch.no_grad():
        prompt = torch.where(torch.arange(W, device=dev)[None] < lens[:, None], seq[:, :W], torch.zeros_like(seq[:, :W]))
        out[rows, lens - 1] = m(prompt, cache=cache).logits[rows, lens - 1].float()
        cache.set_lengths(lens)
        for s in range(steps):
            pos = lens[:, None] + s * CHUNK + t[None, :]  # [B, CHUNK]
            live = pos < SEQ
            n_new = live.sum(1).to(torch.int32)
            tok = seq.gather(1, pos.clamp_max(SEQ - 1))
            h = m._decoder()(tok, cache=cache, n_new=n_new)
            logits = m.lm_head(h).float()
            out[rows[:, None].expand_as(pos)[live], pos[live]] = logits[live]
    return out, cache


@pytest.mark.parametrize("family", FAMILIES)
def test_chunked_teacher_forced_consistency_and_rollback(family, cuda, monkeypatch):
    hip.require()
    m, ref = pair(family, cuda)  # the models of tests/test_generate_gpu.py: no row scales on the LM head
    seq = torch.randint(1, 256, (3, SEQ), generator=torch.Generator().manual_seed(9)).to(cuda)
    lens = torch.tensor(LENS, device=cuda)
    exact = exact_logits(ref, seq)
    with torch.no_grad():
        full = m(seq).logits.float()
    kernels_only(monkeypatch)
    cached, cache = chunked_teacher_forced(m, seq, lens)
    done = ~torch.isnan(cached).any(-1)
    assert bool((done == (torch.arange(SEQ, device=cuda)[None] >= (lens - 1)[:, None])).all())
    assert bool(torch.isfinite(cached[done]).all())
    assert cache.lengths.tolist() == [SEQ] * 3
    e_full = (full - exact).abs().amax(-1)
    e_cached = torch.where(done, (torch.nan_to_num(cached) - exact).abs().amax(-1), torch.zeros_like(e_full))
    ratio = torch.where(done, e_cached / e_full, torch.zeros_like(e_full))
    worst = float(ratio.max())
    b, t = (int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape))
    print(f"[speculative] {family}: chunked / full logit error against fp32, max ratio {worst:.3f} at row {b} position "
          f"{t} (chunked {float(e_cached[b, t]):.3e}, full {float(e_full[b, t]):.3e}); median {float(ratio[done].median()):.3f}")
    assert worst <= MAX_RATIO
    # rollback: two rows lose their last 3 tokens and take them again; the cache geometry of this model has one
    # split at these lengths, where a query's arithmetic depends on its own key range alone
    keep = torch.tensor((SEQ - 3, SEQ, SEQ - 3), device=cuda)
    cache.truncate(keep, SEQ)
    assert cache.lengths.tolist() == keep.tolist() and cache.width == SEQ
    with torch.no_grad():
        h = m._decoder()(seq[:, SEQ - 3:], cache=cache, n_new=(SEQ - keep).to(torch.int32))
        again = m.lm_head(h).float()
    assert cache.lengths.tolist() == [SEQ] * 3
    for b in (0, 2):
        assert torch.equal(again[b], cached[b, SEQ - 3:]), f"{family}: row {b}'s re-fed logits differ from the first pass"
    fused.check_index_errors(blocking=True)


def decided_prefix(m, ref, out, mask):
    """Per row: the number of leading new tokens of ``out`` [B, T0 + n] whose position is decided -- the fp32 twin's
    top-1 / top-2 margin exceeds 2 MAX_RATIO times the full bf16 forward's logit error there (each of two paths may
    be off by MAX_RATIO errors on each of two logits)."""
    prefix = []
    for b in range(out.shape[0]):
        start = int((mask[b] == 0).sum())  # left padding
        seq = out[b:b + 1, start:]
        exact = exact_logits(ref, seq)[0]
        with torch.no_grad():
            full = m(seq).logits.float()[0]
        at = slice(T0 - start - 1, seq.shape[1] - 1)  # the positions that produce the new tokens
        top = exact[at].topk(2, dim=-1).values
        decided = (top[:, 0] - top[:, 1]) > 2 * MAX_RATIO * (full[at] - exact[at]).abs().amax(-1)
        und = (~decided).nonzero()
        prefix.append(int(und[0]) if len(und) else decided.shape[0])
    return prefix


_PLAIN = {}


def plain_run(family, device):
    """(ids, mask, plain greedy output, decided prefix per row), computed once and left unchanged."""
    if family not in _PLAIN:
        m, ref = target(family, device)
        ids, mask = prompts(family, device)
        free = m.generate(ids, attention_mask=mask, max_new_tokens=NEW)
        _PLAIN[family] = (ids, mask, free, decided_prefix(m, ref, free, mask))
    return _PLAIN[family]


def assert_same_where_decided(got, exp, prefix, name):
    for b, p in enumerate(prefix):
        assert torch.equal(got[b, :T0 + p], exp[b, :T0 + p]), (name, b, p, got[b, T0:], exp[b, T0:])


@pytest.mark.parametrize("family", FAMILIES)
def test_plain_greedy_has_a_decided_prefix(family, cuda):
    hip.require()
    prefix = plain_run(family, cuda)[3]
    free = plain_run(family, cuda)[2]
    distinct = [len(set(free[b, T0:T0 + p].tolist())) for b, p in enumerate(prefix)]
    print(f"[speculative] {family}: decided prefix of the plain greedy run per row {prefix} of {NEW}, distinct tokens in "
          f"it {distinct}")
    assert min(prefix) >= MIN_PREFIX, (f"{family}: the compared prefix {prefix} covers fewer than {MIN_PREFIX} of the "
                                       f"{NEW} new tokens; choose another seed (SEEDS)")


@pytest.mark.parametrize("family", FAMILIES)
def test_speculative_equals_plain_greedy_where_decided(family, cuda, monkeypatch):
    hip.require()
    kernels_only(monkeypatch)
    m, _ = target(family, cuda)
    ids, mask, free, prefix = plain_run(family, cuda)
    assert min(prefix) >= MIN_PREFIX, f"{family}: compared prefix {prefix}"
    for name, a in assistants(family, cuda).items():
        out = m.generate(ids, attention_mask=mask, max_new_tokens=NEW, assistant_model=a, return_dict_in_generate=True)
        assert out.sequences.shape == free.shape and torch.equal(out.sequences[:, :T0], ids)
        assert_same_where_decided(out.sequences, free, prefix, f"{family} / {name}")
        print(f"[speculative] {family} / {name}: rounds {out.rounds}, accepted {out.accepted.tolist()}")
        if name == "self" and min(prefix) == NEW:  # every draft is the target's own decided choice
            full, rest = divmod(NEW - 1, 6)
            assert out.rounds == full + (rest > 0) and out.accepted.tolist() == [full * 5 + rest] * 3
    for k in (1, 4, 7):
        out = m.generate(ids, attention_mask=mask, max_new_tokens=NEW, assistant_model=assistants(family, cuda)["one layer"],
                         num_assistant_tokens=k)
        assert_same_where_decided(out, free, prefix, f"{family} / k = {k}")
    fused.check_index_errors(blocking=True)


@pytest.mark.parametrize("family", FAMILIES)
def test_eos_and_pad(family, cuda, monkeypatch):
    hip.require()
    kernels_only(monkeypatch)
    m, _ = target(family, cuda)
    ids, mask, free, prefix = plain_run(family, cuda)
    eos = int(free[1, T0 + 2])  # row 1 stops at its third new token
    plain = m.generate(ids, attention_mask=mask, max_new_tokens=NEW, eos_token_id=eos, pad_token_id=255)
    for name, a in assistants(family, cuda).items():
        out = m.generate(ids, attention_mask=mask, max_new_tokens=NEW, eos_token_id=eos, pad_token_id=255, assistant_model=a)
        # the same comparison rule: a row is compared up to its first undecided position, and the widths only when
        # every row is decided up to the step at which the last row finished
        n = min(out.shape[1], plain.shape[1]) - T0
        assert_same_where_decided(out, plain, [min(p, n) for p in prefix], f"{family} / {name} with EOS")
        if min(prefix) >= plain.shape[1] - T0:
            assert out.shape == plain.shape, (family, name)
        assert bool((out[1, T0 + 3:] == 255).all())


def test_errors(cuda):
    hip.require()
    m, _ = target("llama", cuda)
    a = assistants("llama", cuda)["one layer"]
    ids, mask = prompts("llama", cuda)
    with pytest.raises(ValueError, match="do_sample=False"):
        m.generate(ids, max_new_tokens=4, assistant_model=a, do_sample=True)
    with pytest.raises(ValueError, match="num_beams=1"):
        m.generate(ids, max_new_tokens=4, assistant_model=a, num_beams=2)
    with pytest.raises(ValueError, match="num_assistant_tokens"):
        m.generate(ids, max_new_tokens=4, assistant_model=a, num_assistant_tokens=8)
    other = L.LlamaForCausalLM(transformers.LlamaConfig(**{**_llama_kw(1), "vocab_size": 320})).eval().to(cuda, torch.bfloat16)
    with pytest.raises(ValueError, match="vocabulary"):
        m.generate(ids, max_new_tokens=4, assistant_model=other)
