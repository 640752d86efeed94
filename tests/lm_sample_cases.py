"""Shared by the LM-head sampling tests: the cases, the fp64 form of csrc/lm_sample.hip's contract and the
conditions any implementation's (ids, lse, floor, kept) must meet against it."""
import functools

import torch

import numerics as nm
from distributed_lion_pytorch_amd.ops.reference import _M32, _mix32, sr_key

VOCABS = (5, 64, 513, 4099, 32003)
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
SETTINGS = ((1.0, 0, 1.0), (0.7, 50, 1.0), (1.3, 0, 0.9), (0.8, 40, 0.95), (1.0, 1, 1.0), (1.0, 0, 1e-6),
            (1.0, "v+3", 1.0))  # (temperature, top_k, top_p)
KEY = sr_key(11, 2)


def inv_temperature(t):
    return torch.tensor(1.0 / t, dtype=torch.float32).item()


def rows(n, v, dtype, seed=0):
    """4 * randn rows [n, v rounded up to 8] with large finite values and NaN in the pad columns."""
    g = torch.Generator().manual_seed(seed * 1000003 + 31 * v + n)
    x = 4 * torch.randn(n, (v + 7) // 8 * 8, generator=g)
    x[:, v:] = 3e4
    x[:, v + 1::2] = float("nan")
    return x.to(dtype)


def reference(x, v, inv_t, top_k, key):
    """fp64 (s, top-k survivors, s + g): s is the fp32 product promoted (-inf where NaN), g the Gumbel noise of
    the hash evaluated on int64 tensors."""
    s = (x[:, :v].float().cpu() * torch.tensor(inv_t, dtype=torch.float32)).double()
    s = torch.where(torch.isnan(s), torch.full_like(s, float("-inf")), s)
    surv = s > float("-inf")
    if 1 <= top_k < v:
        surv &= s >= torch.topk(s, top_k, dim=1).values[:, -1:]
    col, row = torch.arange(v)[None, :], torch.arange(x.shape[0])[:, None]
    n = _mix32((_mix32((col ^ key) & _M32) + row * 0x9E3779B1 + 0x85EBCA6B) & _M32) >> 8
    g = -torch.log(-torch.log((n.double() + 0.5) * 2.0 ** -24))
    return s, surv, s + g


@functools.lru_cache(maxsize=None)
def case(n, v, dtype, setting):
    """(x, inv_t, top_k, top_p, reference) of one case, computed once."""
    t, k, p = setting
    k = v + 3 if k == "v+3" else k
    x = rows(n, v, dtype)
    return x, inv_temperature(t), k, p, reference(x, v, inv_temperature(t), k, KEY)


def check(out, x, v, inv_t, top_k, top_p, ref, name):
    """The issue's conditions on (ids, lse, floor, kept); returns per row (floor is forced, token is decided)."""
    ids, lse, floor, kept = (o.cpu() for o in out)
    s, surv, score = ref
    nm.assert_elems_close(lse, torch.logsumexp(s, -1), 1e-5, 1e-5, f"{name} lse")
    tau = 2.0 ** -24 * (v + 8)
    delta = 8 * 2.0 ** -24 * (float(s[s > float("-inf")].abs().max()) + 32)
    stats = []
    for r in range(x.shape[0]):
        sv = s[r][surv[r]]
        vals, inv = torch.unique(sv, return_inverse=True)  # ascending value classes
        mass = torch.zeros_like(vals).index_add_(0, inv, (sv - sv.max()).exp())
        upto = mass.cumsum(0) / mass.sum()
        ok = (upto - mass / mass.sum() <= 1 - top_p + tau) & (upto > 1 - top_p - tau)
        f = float(floor[r])
        at = (vals == f).nonzero()
        assert at.numel() == 1, f"{name} row {r}: floor {f} is no surviving value of the row"
        assert bool(ok[at[0, 0]]), f"{name} row {r}: floor {f} outside the mass bound"
        if top_p == 1.0:
            assert f == float(vals[0]), f"{name} row {r}: the top-k threshold is exact"
        live = surv[r] & (s[r] >= f)
        assert int(kept[r]) == int(live.sum()), f"{name} row {r}: kept {int(kept[r])} != {int(live.sum())}"
        tok = int(ids[r])
        assert 0 <= tok < v and bool(live[tok]), f"{name} row {r}: token {tok} did not survive"
        best = score[r][live].topk(min(2, int(live.sum()))).values
        assert float(score[r, tok]) >= float(best[0]) - delta, f"{name} row {r}: {score[r, tok]} < {best[0]} - {delta}"
        if top_k == 1 and vals.numel() == 1 and int(surv[r].sum()) == 1:
            assert tok == int(s[r].argmax()), f"{name} row {r}: top_k = 1 is the argmax"
        if top_p == 1e-6 and float(mass[-1] / mass.sum()) > 1e-3:
            assert int(kept[r]) == int((sv == vals[-1]).sum()), f"{name} row {r}: top_p -> 0 keeps the maximum only"
        stats.append((int(ok.sum()) == 1 or top_p == 1.0, best.numel() == 1 or float(best[0] - best[1]) > 2 * delta))
    return stats
