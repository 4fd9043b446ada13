"""A second, O(B log B) numpy oracle of the in-batch GAUC counts, for lists the quadratic tests/_auc_oracle.py cannot afford, and the numpy
restatement of what the sort route's kernels key and tile by (csrc/pairwise_auc_sort.hip).  It calls nothing of rec_now_amd.

Oracle.  Written from `searchsorted` on each lower class's sorted scores -- not from prefix scans, which is how the kernels do it.  The classes
are the label levels of the definition (binary rule: label > th or not; graded rule: the distinct non-NaN label values).  Per class c' the
rows of the batch are sorted by (list, score), NaN scores last in their list.  For a taking-part row i of class c and every class c' < c:
  `left` - (start of i's list)  = rows of c' in the list with a score below s_i    -> c_i
  `right` - `left`              = rows of c' in the list with a score equal to s_i -> t_i
  (end of the list) - (start)   = rows of c' in the list                           -> n_i
and a NaN score s_i adds to n_i only.  tests/test_auc_sort_cpu.py pins it exactly to `_auc_oracle.counts`."""
import numpy as np

import _auc_oracle as A
from _pair_lists_oracle import list_ids, rows_of_lists


def classes(labels, take, pos_neg_th=None):
    """(class per row as int64, -1 for a row without one; number of classes)"""
    y = np.asarray(labels).reshape(-1).astype(np.float32)
    cls = np.full(y.size, -1, dtype=np.int64)
    with np.errstate(invalid='ignore'):
        if pos_neg_th is not None:
            cls[take] = (y[take] > np.float32(pos_neg_th)).astype(np.int64)
            return cls, 2
        ok = take & ~np.isnan(y)
        values = np.unique(y[ok])                    # -0.0 and +0.0 are one value
        cls[ok] = np.searchsorted(values, y[ok])
        return cls, int(values.size)


def counts(scores, labels, groups, mask=None, pos_neg_th=None):
    """`_auc_oracle.Counts` of the batch (per row n_i, c_i, t_i; the lists; per list N, C, T, R and the AUC), in O(classes x B log B)"""
    s = np.asarray(scores).reshape(-1).astype(np.float32)
    B = s.size
    take = np.ones(B, dtype=bool) if mask is None else np.asarray(mask).reshape(-1).astype(bool)
    lid = list_ids(groups) if B else np.zeros(0, dtype=np.int64)
    lists = rows_of_lists(lid)
    cls, n_cls = classes(labels, take, pos_neg_th)
    nan = np.isnan(s)
    values = np.unique(s[~nan])                      # -0.0 and +0.0 are one score
    M = int(values.size) + 1                         # ranks 0 .. M - 2; M - 1 is kept for NaN: behind every score of its list
    rank = np.where(nan, M - 1, np.searchsorted(values, np.where(nan, 0, s))).astype(np.int64)
    key = lid * M + rank
    row_n, row_c, row_t = (np.zeros(B, dtype=np.int64) for _ in range(3))
    for lower in range(n_cls - 1):
        keys = np.sort(key[cls == lower])
        i = np.flatnonzero(cls > lower)
        start = np.searchsorted(keys, lid[i] * M, side='left')
        end = np.searchsorted(keys, (lid[i] + 1) * M, side='left')
        left = np.searchsorted(keys, key[i], side='left')
        right = np.searchsorted(keys, key[i], side='right')
        row_n[i] += end - start
        row_c[i] += np.where(nan[i], 0, left - start)
        row_t[i] += np.where(nan[i], 0, right - left)
    n_list = len(lists)
    N, C, T = (np.bincount(lid, weights=v, minlength=n_list).astype(np.int64) for v in (row_n, row_c, row_t))       # (exact: far below 2**53)
    R = np.bincount(lid, weights=take, minlength=n_list).astype(np.int64)
    auc = np.array([A.list_auc(N[g], C[g], T[g]) if N[g] > 0 else np.nan for g in range(n_list)], dtype=np.float64)
    for arr in (row_n, row_c, row_t, N, C, T, R, auc):
        arr.setflags(write=False)
    return A.Counts(row_n, row_c, row_t, lid, lists, N, C, T, R, auc)


# ---- what the kernels key and tile by ------------------------------------------------------------------------------------------------------
NAN_KEY = 0xffffffff


def score_key(scores):
    """the canonical uint32 key of a float32 score: ascending with the score, -0.0 and +0.0 share one, every NaN has the one largest"""
    s = np.asarray(scores).reshape(-1).astype(np.float32)
    u = s.view(np.uint32).astype(np.int64)
    key = np.where(u & 0x80000000, 0xffffffff - u, u | 0x80000000)
    key = np.where(s == 0, 0x80000000, key)
    return np.where(np.isnan(s), NAN_KEY, key).astype(np.int64)


def sorted_layout(list_id, scores):
    """the (list, score key) order: (rows in that order, list per position, key per position, run per position); ties keep the row order"""
    key = score_key(scores)
    lid = np.asarray(list_id).astype(np.int64)
    order = np.lexsort((np.arange(lid.size), key, lid))
    l, k = lid[order], key[order]
    head = np.ones(lid.size, dtype=bool)
    head[1:] = (l[1:] != l[:-1]) | (k[1:] != k[:-1])
    return order, l, k, np.cumsum(head) - 1
