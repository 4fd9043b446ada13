"""fp64 oracle of the in-batch sampled-softmax loss WITH EXTRA NEGATIVES (rec_now_amd/rec_block/in_batch_softmax.py, the `extra_*`
arguments), written as the loops of the definition: per row, per candidate -- the batch columns, then the extras -- never a matrix
expression.  Plus the (B, B + N) torch composition a user writes without the fused loss, and the inputs the CPU and GPU test files share."""
import math

import numpy as np

from _in_batch_softmax_oracle import CONFIGS, _flat, make_case  # noqa: F401


def in_batch_softmax_extra_oracle(query, item, extra_item, item_ids=None, log_q=None, temperature=1.0, mask=None, extra_item_ids=None,
                                  extra_log_q=None, extra_mask=None, remove_accidental_hits=True):
    """dict(lse, pos, row_loss (B,), loss, n, dq, dv (B, D), de (N, D), p (B, B + N) with 0 off the candidates): everything fp64.
    lse and pos are NaN and row_loss 0 where the row does not take part."""
    q, v, x = (np.asarray(t, dtype=np.float64) for t in (query, item, extra_item))
    (B, D), N = q.shape, x.shape[0]
    ids, lq, mk = _flat(item_ids, np.int64), _flat(log_q, np.float64), _flat(mask, np.float64)
    xids, xlq, xmk = _flat(extra_item_ids, np.int64), _flat(extra_log_q, np.float64), _flat(extra_mask, np.float64)
    tau = float(temperature)
    on = [mk is None or mk[i] != 0 for i in range(B)]
    xon = [xmk is None or xmk[k] != 0 for k in range(N)]
    n = sum(on)
    lse, pos, row_loss = np.full(B, np.nan), np.full(B, np.nan), np.zeros(B)
    cands = [[] for _ in range(B)]
    for i in range(B):
        if not on[i]:
            continue
        for j in range(B):                                           # the batch columns
            hit = remove_accidental_hits and ids is not None and ids[j] == ids[i]
            if j == i or (on[j] and not hit):
                s = float(np.dot(q[i], v[j])) / tau - (lq[j] if lq is not None else 0.0)
                cands[i].append((j, s))
                if j == i:
                    pos[i] = s
        for k in range(N):                                           # the extras: candidates only, never the positive
            hit = remove_accidental_hits and ids is not None and xids is not None and xids[k] == ids[i]
            if xon[k] and not hit:
                s = float(np.dot(q[i], x[k])) / tau - (xlq[k] if xlq is not None else 0.0)
                cands[i].append((B + k, s))
        mx = max(s for _, s in cands[i])
        lse[i] = mx + math.log(math.fsum(math.exp(s - mx) for _, s in cands[i]))
        row_loss[i] = lse[i] - pos[i]
    loss = math.fsum(row_loss[i] for i in range(B) if on[i]) / n if n > 0 else 0.0
    dq, dv, de, p = np.zeros((B, D)), np.zeros((B, D)), np.zeros((N, D)), np.zeros((B, B + N))
    for i in range(B):
        for j, s in cands[i]:
            p[i, j] = math.exp(s - lse[i])
            w = (p[i, j] - (1.0 if j == i else 0.0)) / (n * tau)
            if j < B:
                dq[i] += w * v[j]
                dv[j] += w * q[i]
            else:
                dq[i] += w * x[j - B]
                de[j - B] += w * q[i]
    return dict(lse=lse, pos=pos, row_loss=row_loss, loss=loss, n=n, dq=dq, dv=dv, de=de, p=p)


def composition_extra(query, item, extra_item, item_ids=None, log_q=None, temperature=1.0, mask=None, extra_item_ids=None,
                      extra_log_q=None, extra_mask=None, remove_accidental_hits=True):
    """The torch restatement a user writes without the fused loss, in the dtype of `query`: cat + (B, B + N) logits + masked_fill +
    logsumexp.  (loss, lse, pos); differentiable in query, item and extra_item."""
    import torch
    B, N = query.shape[0], extra_item.shape[0]
    logits = query @ torch.cat([item, extra_item]).T / temperature
    if log_q is not None:
        logits = logits - torch.cat([log_q.reshape(-1), extra_log_q.reshape(-1)]).reshape(1, -1).to(logits.dtype)
    eye = torch.cat([torch.eye(B, dtype=torch.bool), torch.zeros(B, N, dtype=torch.bool)], dim=1)
    on = torch.ones(B, dtype=torch.bool) if mask is None else mask.reshape(-1) != 0
    xon = torch.ones(N, dtype=torch.bool) if extra_mask is None else extra_mask.reshape(-1) != 0
    drop = ~torch.cat([on, xon])[None, :].expand(B, B + N)
    if item_ids is not None and remove_accidental_hits:
        drop = drop | (torch.cat([item_ids.reshape(-1), extra_item_ids.reshape(-1)])[None, :] == item_ids.reshape(-1)[:, None])
    logits = logits.masked_fill(drop & ~eye, float('-inf'))
    lse = torch.logsumexp(logits, dim=1)
    pos = torch.diagonal(logits[:, :B])
    rows = (lse - pos)[on]
    loss = rows.mean() if rows.numel() > 0 else logits.sum() * 0.0
    return loss, lse, pos


def make_extra_case(B, N, D, config, rows_tile, extras_tile=32, seed=0):
    """make_case(B, D, config, rows_tile) plus N extras: rows from the same distribution and scale; 'ids': extra ids drawn from the batch's
    B / 4 id values, so that every row has hits among the extras (N permitting); 'log_q': extra_log_q = log U(0.05, 1); 'mask': an extra_mask
    that removes the first `extras_tile` extras as a whole when N is longer than that, and a fifth of the rest."""
    c = make_case(B, D, config, rows_tile, seed=seed)
    rng = np.random.default_rng(77 + 1000 * B + 10 * D + 100003 * N + CONFIGS.index(config) + 100000 * seed)
    scale = D ** -0.25 * (0.7 if D > 64 else 1.0)
    c.update(extra_item=(rng.normal(size=(N, D)) * scale).astype(np.float32), extra_item_ids=None, extra_log_q=None, extra_mask=None)
    if config in ('log_q', 'all'):
        c['extra_log_q'] = np.log(rng.uniform(0.05, 1.0, N)).astype(np.float32)
    if config in ('ids', 'all'):
        c['extra_item_ids'] = rng.integers(0, max(B // 4, 1), N).astype(np.int64) * 7919 - 3
    if config in ('mask', 'all'):
        m = rng.random(N) >= 0.2
        if N > extras_tile:
            m[:extras_tile] = False
        c['extra_mask'] = m
    return c


EXTRA_KEYS = ('extra_item_ids', 'extra_log_q', 'extra_mask')


def oracle_of(case, **over):
    """The oracle on a make_extra_case dict."""
    c = dict(case, **over)
    return in_batch_softmax_extra_oracle(c['query'], c['item'], c['extra_item'], c['item_ids'], c['log_q'], c['temperature'], c['mask'],
                                         c['extra_item_ids'], c['extra_log_q'], c['extra_mask'])


# The shapes (B, N, D) of the GPU tests, from recnow_ibs_tile: R = 64 owner rows, T = 32 streamed rows (both files assert the library agrees).
R, T = 64, 32
SHAPES = [(1, 1, 1), (2, 31, 3), (33, 32, 8), (64, 33, 33), (65, 1, 64), (31, 65, 127), (129, 97, 128), (197, 129, 64), (32, 130, 16)]


def shape_case(B, N, D, config):
    """The inputs of one GPU test shape: the batch mask removes a workgroup's rows as a whole where the batch has three of them, else a wave's."""
    return make_extra_case(B, N, D, config, R if B >= 3 * R else T, T)
