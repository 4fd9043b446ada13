"""fp64 oracle of the in-batch sampled-softmax loss (rec_now_amd/rec_block/in_batch_softmax.py), written as the loops of the definition:
per row, per candidate, never a matrix expression.  Plus the inputs the CPU and GPU test files share."""
import math

import numpy as np


def _flat(a, dtype):
    return None if a is None else np.asarray(a, dtype=dtype).reshape(-1)


def in_batch_softmax_oracle(query, item, item_ids=None, log_q=None, temperature=1.0, mask=None, remove_accidental_hits=True):
    """dict(lse, pos, row_loss (B,), loss, n, dq, dv (B, D), p (B, B) with 0 off the candidates): everything fp64.
    lse and pos are NaN and row_loss 0 where the row does not take part."""
    q, v = np.asarray(query, dtype=np.float64), np.asarray(item, dtype=np.float64)
    B, D = q.shape
    ids, lq, mk = _flat(item_ids, np.int64), _flat(log_q, np.float64), _flat(mask, np.float64)
    tau = float(temperature)
    on = [mk is None or mk[i] != 0 for i in range(B)]
    n = sum(on)
    lse, pos, row_loss = np.full(B, np.nan), np.full(B, np.nan), np.zeros(B)
    cands = [[] for _ in range(B)]
    for i in range(B):
        if not on[i]:
            continue
        for j in range(B):
            hit = remove_accidental_hits and ids is not None and ids[j] == ids[i]
            if j == i or (on[j] and not hit):
                s = float(np.dot(q[i], v[j])) / tau - (lq[j] if lq is not None else 0.0)
                cands[i].append((j, s))
                if j == i:
                    pos[i] = s
        mx = max(s for _, s in cands[i])
        lse[i] = mx + math.log(math.fsum(math.exp(s - mx) for _, s in cands[i]))
        row_loss[i] = lse[i] - pos[i]
    loss = math.fsum(row_loss[i] for i in range(B) if on[i]) / n if n > 0 else 0.0
    dq, dv, p = np.zeros((B, D)), np.zeros((B, D)), np.zeros((B, B))
    for i in range(B):
        for j, s in cands[i]:
            p[i, j] = math.exp(s - lse[i])
            w = (p[i, j] - (1.0 if j == i else 0.0)) / (n * tau)
            dq[i] += w * v[j]
            dv[j] += w * q[i]
    return dict(lse=lse, pos=pos, row_loss=row_loss, loss=loss, n=n, dq=dq, dv=dv, p=p)


def composition(query, item, item_ids=None, log_q=None, temperature=1.0, mask=None, remove_accidental_hits=True):
    """The torch restatement a user writes today, in the dtype of `query` (rows that do not take part deleted from the mean, their columns
    from every other row): (loss, lse, pos).  Differentiable; forms the (B, B) logits."""
    import torch
    B = query.shape[0]
    logits = query @ item.T / temperature
    if log_q is not None:
        logits = logits - log_q.reshape(1, -1).to(logits.dtype)
    eye = torch.eye(B, dtype=torch.bool)
    on = torch.ones(B, dtype=torch.bool) if mask is None else mask.reshape(-1) != 0
    drop = ~on[None, :].expand(B, B)
    if item_ids is not None and remove_accidental_hits:
        ids = item_ids.reshape(-1)
        drop = drop | (ids[None, :] == ids[:, None])
    logits = logits.masked_fill(drop & ~eye, float('-inf'))
    lse = torch.logsumexp(logits, dim=1)
    pos = torch.diagonal(logits)
    rows = (lse - pos)[on]
    loss = rows.mean() if rows.numel() > 0 else logits.sum() * 0.0
    return loss, lse, pos


CONFIGS = ('plain', 'log_q', 'ids', 'mask', 'all')


def make_case(B, D, config, rows_tile, seed=0):
    """Inputs of one test case as numpy arrays: dict(query, item, item_ids, log_q, mask, temperature).  Logits of a few units at the most and
    no trivially classified row: entries N(0, 1) / D^(1/4) (the dot product of two rows has unit variance; half that above D = 64), and a temperature that grows with
    D between 0.5 and 2, so that the fp32 rounding of a D-term dot product, divided by it, stays well inside the 1e-6 the tests allow a logit.
    'ids': B / 4 distinct values (accidental hits in every tile of rows);  'mask': a third to a half of the rows removed -- the second tile of
    `rows_tile` rows as a whole when the batch is longer than one tile, and a fifth of the others (three in ten of a shorter batch)."""
    rng = np.random.default_rng(1000 * B + 10 * D + CONFIGS.index(config) + 100000 * seed)
    scale = D ** -0.25 * (0.7 if D > 64 else 1.0)
    c = dict(query=(rng.normal(size=(B, D)) * scale).astype(np.float32), item=(rng.normal(size=(B, D)) * scale).astype(np.float32),
             item_ids=None, log_q=None, mask=None, temperature=0.5 if D <= 8 else (1.0 if D <= 33 else 2.0))
    if config in ('log_q', 'all'):
        c['log_q'] = np.log(rng.uniform(0.05, 1.0, B)).astype(np.float32)
    if config in ('ids', 'all'):
        c['item_ids'] = rng.integers(0, max(B // 4, 1), B).astype(np.int64) * 7919 - 3
    if config in ('mask', 'all'):
        m = rng.random(B) >= (0.2 if B > rows_tile else 0.3)
        if B > rows_tile:
            m[rows_tile:2 * rows_tile] = False
        c['mask'] = m
    return c
