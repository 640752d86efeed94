"""Shared by the LM-head scoring tests: the fp64 / exact-integer reference of
csrc/lm_score.hip's four outputs and the tie rows both test files use."""
import torch


def reference_score(x, labels, v, eps=0.0, zeta=0.0):
    """(row_loss, lse) in fp64 and (pred, rank) as int64 from the stored logits
    x[:, :v]: pred is the first column of the row maximum, rank the number of
    columns with a greater value than the label's plus the equal ones before
    it.  Rows whose label is outside [0, v): loss 0, rank -1."""
    x64 = x[:, :v].double()
    lse = torch.logsumexp(x64, -1)
    valid = (labels >= 0) & (labels < v)
    safe = labels.clamp(0, v - 1)
    tgt = x64.gather(1, safe[:, None])
    row = lse - (1 - eps) * tgt[:, 0] + zeta * lse * lse
    if eps:
        row = row - eps * x64.mean(-1)
    loss = torch.where(valid, row, torch.zeros_like(row))
    cols = torch.arange(v, device=x.device)
    pred = torch.where(x64 == x64.max(-1, keepdim=True).values, cols, cols.new_full((), v)).min(-1).values
    before = (x64 > tgt).sum(-1) + ((x64 == tgt) & (cols < safe[:, None])).sum(-1)
    rank = torch.where(valid, before, torch.full_like(before, -1))
    return loss, lse, pred, rank


def tie_rows(v, vp, dtype, device, threads=512):
    """Logits [R, vp] and labels [R] whose maximum is stored at several columns,
    chosen to straddle element (7 | 8), wave (511 | 512), block-iteration
    (8 threads - 1 | 8 threads) and row-end boundaries of a ``threads``-thread
    kernel that gives each thread 8 consecutive columns per iteration.  Per tie
    set: the label on the first tied column, on the last, and on a non-maximal
    value with an equal value below and above its column; then a {-0.0, +0.0}
    pair in an otherwise negative row, labelled either way, and an ignored row.
    Pad columns hold +1e4, above every real value."""
    g = torch.Generator().manual_seed(v)
    big = 8 * threads
    sets = [[7, 8], [511, 512], [0, big - 1, big], [min(4096, v // 2), v - 1], [big, 3 * big + 5, v - 1]]
    sets = [sorted({c for c in s if c < v}) for s in sets]
    sets = [s for s in sets if len(s) >= 2]
    dup = [3, v // 3, v - 2]
    rows, labels = [], []

    def base():
        return -(3 * torch.rand(vp, generator=g) + 1)  # all in [-4, -1]

    for s in sets:
        for lab in (s[0], s[-1], dup[1]):
            r = base()
            r[s] = 2.0
            r[dup] = -0.5
            rows.append(r)
            labels.append(lab)
    p, q = v // 4, v // 2 + 1
    for lab in (p, q):
        r = base()
        r[p], r[q] = -0.0, 0.0
        rows.append(r)
        labels.append(lab)
    r = base()
    r[sets[0]] = 2.0
    rows.append(r)
    labels.append(-100)
    x = torch.stack(rows)
    x[:, v:] = 1e4
    return x.to(dtype).to(device), torch.tensor(labels, device=device)
