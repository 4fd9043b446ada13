"""GAUC inside the batch: the AUC of every list, averaged over the lists (the metric of the DIN paper), from exact integer pair counts.

Lists and rows.  A list is one segment of `build_segments(groups)`.  Only rows that take part are looked at.  A row takes part when `mask` is
true, or when no mask is given.

Pairs.  For two distinct taking-part rows i, j of one list, (i, j) is a pair:

  - under the graded rule, when `label_i > label_j`.  This is the default, `pos_neg_th=None`, and is the concordance index for graded labels.
    For 0/1 labels it is the AUC.
  - under the binary rule, when `label_i > th and not (label_j > th)`.  This applies when `pos_neg_th=th` is given as a finite float.

Comparisons are float32 and IEEE.  A NaN label is therefore in no pair under the graded rule and is a negative under the binary rule.

Per-row counts.  These are kept by row i as the higher side of the pair, as int32:

  - `n_i` = number of j for which (i, j) is a pair
  - `c_i` = number of pairs with `s_i > s_j`
  - `t_i` = number of pairs with `s_i == s_j`

A NaN score makes both comparisons false, so that pair counts as discordant.  A row that does not take part holds 0, 0, 0.

Per-list counts.  `N`, `C`, `T` are the int64 sums of `n_i`, `c_i`, `t_i` over the list, and `R` is the number of taking-part rows.  The list's
AUC is `(2C + T) / (2N)`, formed in fp64 from the integers, for lists with N > 0.  Lists with N = 0 have no AUC and are left out of every batch
mean.

Batch metric.  The metric is `sum_L w_L AUC_L / sum_L w_L` over the lists with N > 0.  The weight `w_L` depends on `weight=`:

  - `'rows'`: `w_L` = R.  This is the default and is impressions-weighted GAUC.
  - `'pairs'`: `w_L` = N.  This is the pooled share of correctly ordered pairs.
  - `'uniform'`: `w_L` = 1.

The metric is 0 when no list has N > 0.  The sums are fp64 in a fixed order.

Everything is computed by csrc/pairwise_auc.hip (recnow_pair_auc_terms): one compare-only traversal of every segment, integer sums per list,
no host synchronisation, bitwise reproducible.  The walk is quadratic in the length of a list."""
import collections
import math
import numbers

import torch

from .. import _lib
from ._segments import _inputs

_WEIGHT_CODE = {'rows': 0, 'pairs': 1, 'uniform': 2}          # RECNOW_AUC_WEIGHT_* of include/recnow.h


def _check_options(weight, pos_neg_th):
    if not isinstance(weight, str) or weight not in _WEIGHT_CODE:
        raise ValueError("weight must be 'rows', 'pairs' or 'uniform', got %r" % (weight,))
    if pos_neg_th is not None and (isinstance(pos_neg_th, bool) or not isinstance(pos_neg_th, numbers.Real) or not math.isfinite(pos_neg_th)):
        raise ValueError('pos_neg_th must be None or a finite number, got %r' % (pos_neg_th,))


InBatchAUC = collections.namedtuple('InBatchAUC', ['auc', 'n_lists', 'weighted_sum', 'weight_sum'])
AUCTerms = collections.namedtuple('AUCTerms', ['row_pairs', 'row_concordant', 'row_tied', 'list_pairs', 'list_concordant', 'list_tied',
                                               'list_rows'])


def auc_workspace(B, device):
    """The workspace of recnow_pair_auc_terms; a count call in front of it may share it (recnow_pair_auc_workspace_bytes)."""
    return _lib.workspace(_lib.load().recnow_pair_auc_workspace_bytes(B), device)


def _call(seg, scores, labs, m, pos_neg_th, weight, rows, lists, metric):
    P = _lib.ptr
    ws = auc_workspace(seg.B, seg.device)
    _lib.call('recnow_pair_auc_terms', P(scores), P(labs), P(m), P(seg.order), P(seg.seg_id), P(seg.seg_first), seg.B, 0,
              0 if pos_neg_th is None else 1, 0.0 if pos_neg_th is None else float(pos_neg_th), _WEIGHT_CODE[weight],
              *[P(t) for t in rows + lists + metric], P(ws), ws.numel(), _lib.stream())


def in_batch_gauc(outputs, labels, groups, mask=None, pos_neg_th=None, weight='rows', segments=None):
    """InBatchAUC(auc, n_lists, weighted_sum, weight_sum) as 0-dim tensors (float32, int64, float64, float64): the weighted mean of the lists'
    AUC over the lists that have a pair -- 0 when there is none --, the number of such lists, and the mean's numerator and denominator (what
    `dp.global_gauc` sums over the ranks).  No host synchronisation, no gradient.  segments: a precomputed `group_rows(groups)` (`groups` is
    then not looked at)."""
    _check_options(weight, pos_neg_th)
    seg, scores, labs, m = _inputs(outputs, labels, groups, mask, segments)
    dev = seg.device
    auc = torch.empty((), dtype=torch.float32, device=dev)
    n_lists = torch.empty((), dtype=torch.int64, device=dev)
    wsum, wt = (torch.empty((), dtype=torch.float64, device=dev) for _ in range(2))
    _call(seg, scores, labs, m, pos_neg_th, weight, [None] * 3, [None] * 4, [auc, wsum, wt, n_lists])
    return InBatchAUC(auc, n_lists, wsum, wt)


def auc_terms(outputs, labels, groups, mask=None, pos_neg_th=None, segments=None):
    """The counts behind the metric.  `row_pairs`, `row_concordant`, `row_tied`: n_i, c_i, t_i per ORIGINAL row, flat int32 tensors of B
    elements.  `list_pairs`, `list_concordant`, `list_tied`, `list_rows`: N, C, T, R per SEGMENT, int64 tensors of B elements of which only the
    first `n_seg` (the number of lists, `segments.num_segments()`) are meaningful; the entries behind them are not written.  No host
    synchronisation, no gradient."""
    _check_options('rows', pos_neg_th)
    seg, scores, labs, m = _inputs(outputs, labels, groups, mask, segments)
    B, dev = seg.B, seg.device
    rows = [torch.empty(max(B, 1), dtype=torch.int32, device=dev) for _ in range(3)]
    lists = [torch.empty(max(B, 1), dtype=torch.int64, device=dev) for _ in range(4)]
    _call(seg, scores, labs, m, pos_neg_th, 'rows', rows, lists, [None] * 4)
    return AUCTerms(*[t[:B] for t in rows + lists])
