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

Two routes compute the same integers, so every output is bit-identical between them (`route=`):

  - `'walk'` (csrc/pairwise_auc.hip, recnow_pair_auc_terms): one compare-only traversal of every list.  Its cost is the sum of the squared
    list lengths: the route for the short lists of impression data, and the default of `in_batch_gauc` / `auc_terms`.
  - `'sort'` (csrc/pairwise_auc_sort.hip, recnow_pair_auc_sorted_terms): every list is sorted by score and the counts are differences of
    per-class prefix counts.  Its cost is O(B log B) whatever the list lengths: the route for one user with thousands of rows, and for the
    AUC of the whole batch as one list (`in_batch_auc`, which picks it from `AUC_SORT_FROM` rows on).

The 16-value rule of the sort route.  Under the graded rule its classes are the distinct non-NaN label values of the taking-part rows of the
batch, found on the device; up to 16 are supported (the cap of `LabelPairWeightTable`).  The binary rule has two classes and takes any labels.

Poisoning.  Nothing here synchronises the host, so the sort route cannot raise for what only the device knows.  With more than 16 label values
under the graded rule, or when its grouping call reports a grid-barrier time-out, every output is overwritten instead: `auc`, `weighted_sum`
and `weight_sum` are NaN, `n_lists` is -1, and every per-row and per-list count is -1.

No host synchronisation, no gradient, bitwise reproducible on either route."""
import collections
import math
import numbers

import torch

from .. import _lib
from ._segments import Segments, _inputs

_WEIGHT_CODE = {'rows': 0, 'pairs': 1, 'uniform': 2}          # RECNOW_AUC_WEIGHT_* of include/recnow.h


AUC_SORT_FROM = 4096      # rows from which in_batch_auc(route='auto') takes the sort route: set from profiles/pair_auc_sort_bench.txt
AUC_SORT_TILE = 1024      # RECNOW_AUC_SORT_TILE of include/recnow.h: positions per workgroup of the sort route's prefix-count kernels
_ROUTES = ('walk', 'sort')
_ENTRY = {'walk': 'recnow_pair_auc_terms', 'sort': 'recnow_pair_auc_sorted_terms'}
_WS_BYTES = {'walk': 'recnow_pair_auc_workspace_bytes', 'sort': 'recnow_pair_auc_sorted_workspace_bytes'}


def _check_options(weight, pos_neg_th, route='walk', routes=_ROUTES):
    if not isinstance(route, str) or route not in routes:
        raise ValueError('route must be %s, got %r' % (' or '.join(repr(r) for r in routes), route))
    if not isinstance(weight, str) or weight not in _WEIGHT_CODE:
        raise ValueError("weight must be 'rows', 'pairs' or 'uniform', got %r" % (weight,))
    if pos_neg_th is not None and (isinstance(pos_neg_th, bool) or not isinstance(pos_neg_th, numbers.Real) or not math.isfinite(pos_neg_th)):
        raise ValueError('pos_neg_th must be None or a finite number, got %r' % (pos_neg_th,))


InBatchAUC = collections.namedtuple('InBatchAUC', ['auc', 'n_lists', 'weighted_sum', 'weight_sum'])
AUCTerms = collections.namedtuple('AUCTerms', ['row_pairs', 'row_concordant', 'row_tied', 'list_pairs', 'list_concordant', 'list_tied',
                                               'list_rows'])


def auc_workspace(B, device, route='walk'):
    """The workspace of recnow_pair_auc_terms -- a count call in front of it may share it (recnow_pair_auc_workspace_bytes) --, or of
    recnow_pair_auc_sorted_terms (route='sort': recnow_pair_auc_sorted_workspace_bytes)."""
    return _lib.workspace(getattr(_lib.load(), _WS_BYTES[route])(B), device)


def _call(seg, scores, labs, m, pos_neg_th, weight, rows, lists, metric, route='walk'):
    P = _lib.ptr
    ws = auc_workspace(seg.B, seg.device, route)
    _lib.call(_ENTRY[route], P(scores), P(labs), P(m), P(seg.order), P(seg.seg_id), P(seg.seg_first), seg.B, 0,
              0 if pos_neg_th is None else 1, 0.0 if pos_neg_th is None else float(pos_neg_th), _WEIGHT_CODE[weight],
              *[P(t) for t in rows + lists + metric], P(ws), ws.numel(), _lib.stream())


def in_batch_gauc(outputs, labels, groups, mask=None, pos_neg_th=None, weight='rows', segments=None, *, route='walk'):
    """InBatchAUC(auc, n_lists, weighted_sum, weight_sum) as 0-dim tensors (float32, int64, float64, float64): the weighted mean of the lists'
    AUC over the lists that have a pair -- 0 when there is none --, the number of such lists, and the mean's numerator and denominator (what
    `dp.global_gauc` sums over the ranks).  No host synchronisation, no gradient.  segments: a precomputed `group_rows(groups)` (`groups` is
    then not looked at).  route: 'walk' or 'sort' (the module docstring says when to choose which; 'sort' poisons its outputs instead of raising)."""
    _check_options(weight, pos_neg_th, route)
    seg, scores, labs, m = _inputs(outputs, labels, groups, mask, segments)
    return _metric(seg, scores, labs, m, pos_neg_th, weight, route)


def _metric(seg, scores, labs, m, pos_neg_th, weight, route):
    dev = seg.device
    auc = torch.empty((), dtype=torch.float32, device=dev)
    n_lists = torch.empty((), dtype=torch.int64, device=dev)
    wsum, wt = (torch.empty((), dtype=torch.float64, device=dev) for _ in range(2))
    _call(seg, scores, labs, m, pos_neg_th, weight, [None] * 3, [None] * 4, [auc, wsum, wt, n_lists], route)
    return InBatchAUC(auc, n_lists, wsum, wt)


def auc_terms(outputs, labels, groups, mask=None, pos_neg_th=None, segments=None, *, route='walk'):
    """The counts behind the metric.  `row_pairs`, `row_concordant`, `row_tied`: n_i, c_i, t_i per ORIGINAL row, flat int32 tensors of B
    elements.  `list_pairs`, `list_concordant`, `list_tied`, `list_rows`: N, C, T, R per SEGMENT, int64 tensors of B elements of which only the
    first `n_seg` (the number of lists, `segments.num_segments()`) are meaningful; the entries behind them are not written.  No host
    synchronisation, no gradient.  route: as `in_batch_gauc`; a poisoned 'sort' call holds -1 in all B entries of every tensor."""
    _check_options('rows', pos_neg_th, route)
    seg, scores, labs, m = _inputs(outputs, labels, groups, mask, segments)
    return _terms(seg, scores, labs, m, pos_neg_th, route)


def _terms(seg, scores, labs, m, pos_neg_th, route):
    B, dev = seg.B, seg.device
    rows = [torch.empty(max(B, 1), dtype=torch.int32, device=dev) for _ in range(3)]
    lists = [torch.empty(max(B, 1), dtype=torch.int64, device=dev) for _ in range(4)]
    _call(seg, scores, labs, m, pos_neg_th, 'rows', rows, lists, [None] * 4, route)
    return AUCTerms(*[t[:B] for t in rows + lists])


# ---- the whole batch as one list -------------------------------------------------------------------------------------------------------------
def _resolve_route(route, B):
    """'auto' by the number of rows alone: B is the length of the one list, and the host knows it."""
    return ('sort' if B >= AUC_SORT_FROM else 'walk') if route == 'auto' else route


def _one_list(outputs, labels, mask):
    """(segments, scores, labels, mask) of the batch as ONE list, without a grouping call: the identity order, one segment [0, B)."""
    _lib.require_gpu(outputs, 'outputs')
    B, dev = outputs.numel(), outputs.device
    seg = Segments()
    seg.B, seg.device = B, dev
    seg.order = torch.arange(max(B, 1), dtype=torch.int32, device=dev)
    seg.seg_id = torch.zeros(max(B, 1), dtype=torch.int32, device=dev)
    seg.seg_first = torch.full((B + 1,), B, dtype=torch.int32, device=dev)
    seg.seg_first[:1].zero_()            # (a fill launch: an indexed assignment of a host scalar is a host copy, which no stream capture takes)
    seg.super_id = seg.seg_id
    seg.n_seg = torch.full((2,), min(B, 1), dtype=torch.int32, device=dev)
    return _inputs(outputs, labels, None, mask, seg)


def in_batch_auc(outputs, labels, mask=None, pos_neg_th=None, *, route='auto'):
    """The AUC of the whole batch as one list -- under the graded rule (pos_neg_th=None) the concordance index, which is the AUC for 0/1
    labels --: `in_batch_gauc` with one list and weight='pairs'.  InBatchAUC(auc, n_lists, weighted_sum, weight_sum) as 0-dim tensors:
    `weighted_sum` = (2C + T) / 2, `weight_sum` = N, `n_lists` is 1 when the batch holds a pair and else 0 (auc is then 0).  route: 'walk',
    'sort', or 'auto': the sort route from `AUC_SORT_FROM` rows on.  The walk costs B**2 here.  No grouping call, no host synchronisation, no
    gradient.  Not a sum of per-rank parts under data parallelism: pairs cross ranks."""
    _check_options('pairs', pos_neg_th, route, _ROUTES + ('auto',))
    seg, scores, labs, m = _one_list(outputs, labels, mask)
    return _metric(seg, scores, labs, m, pos_neg_th, 'pairs', _resolve_route(route, seg.B))


def auc_batch_terms(outputs, labels, mask=None, pos_neg_th=None, *, route='auto'):
    """`auc_terms` of the whole batch as one list (the counts behind `in_batch_auc`): element 0 of the four per-list tensors is the list's."""
    _check_options('pairs', pos_neg_th, route, _ROUTES + ('auto',))
    seg, scores, labs, m = _one_list(outputs, labels, mask)
    return _terms(seg, scores, labs, m, pos_neg_th, _resolve_route(route, seg.B))
