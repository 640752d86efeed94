"""Shared by the LM-head top-k tests: the stable-sort oracle of csrc/lm_topk.hip's
three outputs, the random case generator and the tie rows every test file uses."""
import torch

from lm_score_cases import tie_rows

THREADS = 512  # kTopkThreads: 8 columns per thread and iteration
BIG = 8 * THREADS


def reference_topk(x, v, k):
    """(values fp32 [N, k], ids int64 [N, k], lse fp64 [N]) of the stored logits
    x[:, :v]: the first k columns of a stable descending sort of the fp32 values
    (greater value first, lower column among equal values; -0.0 == +0.0) and the
    fp64 logsumexp."""
    xf = x[:, :v].float()
    srt, order = torch.sort(xf, dim=1, descending=True, stable=True)
    return srt[:, :k], order[:, :k], torch.logsumexp(xf.double(), -1)


def padded(v):
    return (v + 63) // 64 * 64


def random_rows(n, v, dtype, device, seed=0):
    """2 * randn rows [n, padded(v)] with +1e4 in the pad columns."""
    g = torch.Generator().manual_seed(seed * 1000003 + v)
    x = 2 * torch.randn(n, padded(v), generator=g)
    x[:, v:] = 1e4
    return x.to(dtype).to(device)


def tie_rows_topk(v, vp, dtype, device):
    """Logits [R, vp] (v > 3 * BIG + 5) made of ties, +1e4 in the pad columns:
    - the tie sets of lm_score_cases.tie_rows (element 7|8, wave 511|512,
      block-iteration 4095|4096, row end),
    - a constant row (ids 0..k-1),
    - a row with 3 finite values and the rest -inf,
    - a row whose k-th value (for every k in 2..40) is shared by columns on both
      sides of the block-iteration boundary 4095|4096,
    - a {-0.0, +0.0} pair above everything else, the -0.0 at the lower column.
    Returns (x, index of the first extra row)."""
    x, _ = tie_rows(v, vp, torch.float32, "cpu", threads=THREADS)
    first = x.shape[0]
    g = torch.Generator().manual_seed(v + 1)

    def base():
        return -(3 * torch.rand(vp, generator=g) + 1)  # all in [-4, -1]

    const = torch.full((vp,), 0.5)
    few = torch.full((vp,), float("-inf"))
    few[[v - 1, 5, BIG]] = torch.tensor([1.0, 1.0, -2.0])
    shared = base()
    shared[9] = 3.0  # one value above the 40 tied ones
    shared[BIG - 20:BIG + 20] = 2.0
    zeros = base()
    zeros[v // 4], zeros[v // 2 + 1] = -0.0, 0.0
    extra = torch.stack([const, few, shared, zeros])
    extra[:, v:] = 1e4
    return torch.cat([x, extra]).to(dtype).to(device), first


def check_tie_rows(values, ids, x, v, k, first):
    """The shapes tie_rows_topk promises, on any implementation's output for k."""
    ids = ids.long().cpu()
    assert ids[first].tolist() == list(range(k)), "constant row"
    if k >= 3:
        assert ids[first + 1, :3].tolist() == [5, v - 1, BIG]
        assert ids[first + 1, 3:].tolist() == [c for c in range(v) if c not in (5, BIG)][:k - 3], "-inf columns"
    want = ([9] + list(range(BIG - 20, BIG + 20)))[:k]
    assert ids[first + 2, :len(want)].tolist() == want, "tie across the block-iteration boundary"
    if k >= 2:
        assert ids[first + 3, :2].tolist() == [v // 4, v // 2 + 1], "-0.0 before +0.0"
        got = values[first + 3, :2].cpu()
        assert torch.equal(torch.signbit(got), torch.tensor([True, False])), "values are the stored logits"
