"""Per-list fp64 oracle of listwise_loss_from_batch, without the (G, B) matrices: numpy, O(B log B).

Restates the reference, rec_now/rec_block/listwise_loss_from_batch.py:89-173 (not the kernels):

  lists     tf.unique equality per id tensor (:109): floats with -0.0 == +0.0, equal infinities equal, every NaN alone; integers
            exact.  Several id tensors: a list is the set of rows that agree in every one.  Lists are numbered by first occurrence.
  validity  both tests run on the zero-padded (G, B) row (:135-137):
              has_pos = any member label > float32(th), or 0 > th when the list is shorter than the batch (its padding);
              has_neg = any float32(label) - float32(th) < 0  (the padding of `labels - th` is 0, never below 0).
  row       the members' logits plus (B - n_g) entries of pad_logit (= value_of_masked_logit, or 0 when do_mask_logits=False; :139-140)
  p_i = y_i / sum_g y (:144);  l_g = w_g (lse_g * sum p - sum p s) (:167-169);  loss = mean over valid lists, 0 when there is none (:170-172)
  gradient  d loss / d s_i = w_g (exp(s_i - lse_g) * sum p - p_i) / n_valid inside a valid list, else 0.

tests/test_listwise_oracle_cpu.py pins it to oracle/dense_ref.py (the reference's dense formulation, pinned to its goldens).
"""
import numpy as np


def _codes(ids):
    """One id tensor -> int64 code per row, equal codes <=> tf.unique finds the ids equal."""
    a = np.asarray(ids).reshape(-1)
    n = a.size
    if a.dtype.kind == 'f':
        a = a.astype(np.float64 if a.dtype.itemsize > 4 else np.float32)
        nan = np.isnan(a)
        a = np.where(a == 0, np.zeros((), a.dtype), a)            # -0.0 -> +0.0
        bits = a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)
        _, inv = np.unique(bits, return_inverse=True)
        inv = inv.reshape(-1).astype(np.int64)
        inv[nan] = inv.max(initial=0) + 1 + np.arange(n)[nan]     # every NaN row is a list of its own
        return inv
    _, inv = np.unique(a, return_inverse=True)
    return inv.reshape(-1).astype(np.int64)


def list_index(ids_list):
    """ids_list: one array or a list of arrays of B ids.  Returns (list index of every row, number of lists), lists numbered by
    first occurrence."""
    if not isinstance(ids_list, (list, tuple)):
        ids_list = [ids_list]
    code = None
    for ids in ids_list:
        c = _codes(ids)
        if code is None:
            code = c
        else:                                                      # rows agree in both <=> the pair of codes agrees
            _, code = np.unique(code, return_inverse=True)
            code = code.reshape(-1).astype(np.int64) * (int(c.max(initial=0)) + 1) + c
    _, first, inv = np.unique(code, return_index=True, return_inverse=True)
    rank = np.empty(first.size, dtype=np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(first.size)
    return rank[inv.reshape(-1)], int(first.size)


class ListwiseRef(object):
    __slots__ = ('loss', 'n_valid', 'per_list', 'grad', 'dbase', 'row_list', 'valid', 'n_rows', 'ysum', 'has_pos', 'has_neg', 'row_rank')


def listwise_ref(ids_list, labels, logits, weights=None, pad_logit=-1e9, pos_neg_th=0.5):
    """Returns a ListwiseRef:
      loss, n_valid; per_list (n_valid,) weighted losses of the valid lists in first-occurrence order; grad (B,) = d loss / d logits;
      dbase (B,) = d per_list[rank of the row's list] / d logits (the do_reduce=False gradient before the upstream vector);
      row_list (B,) list index of every row; valid (G,) flags; n_rows, ysum, has_pos, has_neg (G,); row_rank (B,) valid rank or -1.
    weights: one per VALID list in first-occurrence order, or None."""
    y32 = np.asarray(labels).reshape(-1).astype(np.float32)
    s = np.asarray(logits).reshape(-1).astype(np.float64)
    B = s.size
    row_list, G = list_index(ids_list)
    assert row_list.size == B and y32.size == B
    th32 = np.float32(pos_neg_th)
    y = y32.astype(np.float64)
    n = np.bincount(row_list, minlength=G)
    short = n < B
    has_pos = np.bincount(row_list, weights=(y32 > th32), minlength=G) > 0
    if 0.0 > float(th32):
        has_pos = has_pos | short
    has_neg = np.bincount(row_list, weights=((y32 - th32) < np.float32(0)), minlength=G) > 0
    valid = has_pos & has_neg
    mx = np.full(G, -np.inf)
    np.maximum.at(mx, row_list, s)
    mx = np.where(short, np.maximum(mx, pad_logit), mx)
    z = np.bincount(row_list, weights=np.exp(s - mx[row_list]), minlength=G) + np.where(short, (B - n) * np.exp(pad_logit - mx), 0.0)
    lse = mx + np.log(z)
    ysum = np.bincount(row_list, weights=y, minlength=G)
    with np.errstate(divide='ignore', invalid='ignore'):
        p = y / ysum[row_list]
    p = np.where(valid[row_list], p, 0.0)
    psum = np.bincount(row_list, weights=p, minlength=G)
    pdot = np.bincount(row_list, weights=p * s, minlength=G)
    n_valid = int(valid.sum())
    vrank = np.where(valid, np.cumsum(valid) - 1, -1)
    w = np.ones(G)
    if weights is not None:
        wv = np.asarray(weights, dtype=np.float64).reshape(-1)
        assert wv.size == n_valid, 'one weight per valid list'
        w[valid] = wv
    lg = w * (lse * psum - pdot)
    r = ListwiseRef()
    r.per_list = lg[valid]
    r.n_valid = n_valid
    r.loss = float(r.per_list.mean()) if n_valid > 0 else 0.0
    r.dbase = np.where(valid[row_list], w[row_list] * (np.exp(s - lse[row_list]) * psum[row_list] - p), 0.0)
    r.grad = r.dbase / max(n_valid, 1)
    r.row_list, r.valid, r.n_rows, r.ysum, r.has_pos, r.has_neg = row_list, valid, n, ysum, has_pos, has_neg
    r.row_rank = vrank[row_list]
    return r
