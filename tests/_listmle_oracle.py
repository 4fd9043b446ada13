"""Per-list fp64 oracle of listmle_loss_from_batch: numpy, list by list, from the definitions (not from the kernels).

  lists        `list_index` of tests/_listwise_oracle.py: tf.unique equality, numbered by first occurrence.
  taking part  mask is None or non-zero there, and the label is not NaN.
  permutation  the taking-part rows of a list by label descending (-0.0 == +0.0), ties by ascending row index; n rows, logits s_1 .. s_n.
  valid        n >= 2 and at least two distinct label values among the taking-part rows.
  K            n if topn is None, else min(topn, n).
  loss         l = sum_{p <= K} (lse_p - s_p), lse_p = log sum_{q >= p} exp(s_q); / K with list_mean; times the weight of the list's valid rank.
  gradient     dl/ds_q = exp(s_q + logA_q) - [q <= K], logA_q = log sum_{p <= min(q, K)} exp(-lse_p); same factors.
  reduction    loss = mean over the valid lists (0 when there is none); grad = dbase / n_valid.
  non-finite   a non-finite logit of a taking-part row: the list's loss is NaN here (the device's is merely non-finite) and the gradient of
               every taking-part row of the list is NaN.

tests/test_listmle_cpu.py pins it to a hand-worked list, to a brute force over softmax choices and to torch.logcumsumexp autograd.
"""
import numpy as np

from _listwise_oracle import list_index


class ListMLERef(object):
    __slots__ = ('loss', 'n_valid', 'per_list', 'grad', 'dbase', 'position', 'lse', 'valid', 'list_loss', 'row_list', 'row_rank', 'n_rows', 'K')


def _lse(x):
    """log sum exp of a non-empty fp64 vector."""
    m = np.max(x)
    return m + np.log(np.sum(np.exp(x - m)))


def listmle_ref(ids_list, labels, logits, weights=None, mask=None, topn=None, list_mean=False):
    """Returns a ListMLERef:
      loss, n_valid; per_list (n_valid,) the valid lists' losses (weight and 1/K applied) in first-occurrence order; grad (B,) = d loss / d logits;
      dbase (B,) = d per_list[rank of the row's list] / d logits; position (B,) place in the permutation or -1; lse (B,) lse_p of the row's place
      or NaN; valid (G,), list_loss (G,) unweighted and before 1/K, n_rows (G,) taking-part rows, K (G,); row_list (B,), row_rank (B,) valid rank
      or -1.  weights: one per VALID list in first-occurrence order, or None."""
    y32 = np.asarray(labels).reshape(-1).astype(np.float32)
    s = np.asarray(logits).reshape(-1).astype(np.float32).astype(np.float64)
    B = s.size
    row_list, G = list_index(ids_list) if B > 0 else (np.zeros(0, np.int64), 0)
    part = ~np.isnan(y32)
    if mask is not None:
        part &= np.asarray(mask).reshape(-1) != 0
    r = ListMLERef()
    r.position = np.full(B, -1, dtype=np.int64)
    r.lse = np.full(B, np.nan)
    r.valid = np.zeros(G, dtype=bool)
    r.list_loss = np.zeros(G)
    r.n_rows = np.zeros(G, dtype=np.int64)
    r.K = np.zeros(G, dtype=np.int64)
    base = np.zeros(B)                                   # d list_loss / d logits
    by_list = np.argsort(row_list, kind='stable')
    bounds = np.concatenate([[0], np.cumsum(np.bincount(row_list, minlength=G))]).astype(np.int64)
    for g in range(G):
        rows = by_list[bounds[g]:bounds[g + 1]]
        rows = rows[part[rows]]                          # ascending row index
        n = rows.size
        r.n_rows[g] = n
        if n == 0:
            continue
        y = y32[rows].astype(np.float64) + 0.0           # -0.0 + 0.0 = +0.0
        perm = rows[np.argsort(-y, kind='stable')]       # label descending, ties by ascending row index
        sp = s[perm]
        K = n if topn is None else min(int(topn), n)
        r.K[g] = K
        r.valid[g] = n >= 2 and np.unique(y).size >= 2
        lse = np.empty(n)
        with np.errstate(all='ignore'):
            for p in range(n):
                lse[p] = _lse(sp[p:])
            r.position[perm] = np.arange(n)
            r.lse[perm] = lse
            if not np.all(np.isfinite(sp)):
                r.list_loss[g] = np.nan
                base[perm] = np.nan
                continue
            r.list_loss[g] = float(np.sum(lse[:K] - sp[:K]))
            for q in range(n):
                logA = _lse(-lse[:min(q + 1, K)])
                base[perm[q]] = np.exp(sp[q] + logA) - (1.0 if q < K else 0.0)
    r.n_valid = int(r.valid.sum())
    vrank = np.where(r.valid, np.cumsum(r.valid) - 1, -1)
    w = np.ones(G)
    if weights is not None:
        wv = np.asarray(weights, dtype=np.float64).reshape(-1)
        assert wv.size == r.n_valid, 'one weight per valid list'
        w[r.valid] = wv
    scale = w / np.maximum(r.K, 1) if list_mean else w
    r.per_list = (scale * r.list_loss)[r.valid]
    r.loss = float(np.mean(r.per_list)) if r.n_valid > 0 else 0.0
    r.row_list = row_list
    r.row_rank = vrank[row_list] if B > 0 else np.zeros(0, np.int64)
    with np.errstate(invalid='ignore'):
        r.dbase = np.where(r.valid[row_list] & part, scale[row_list] * base, 0.0) if B > 0 else np.zeros(0)
    r.grad = r.dbase / max(r.n_valid, 1)
    return r
