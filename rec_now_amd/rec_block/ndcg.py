"""NDCG inside the batch: the LambdaRank pair weight |delta NDCG| for `pairwise_loss`, and the in-batch NDCG metric.

A list is one segment of `build_segments(groups)`: the rows that agree in every group tensor.  Only rows that take part (`mask` true, or no
mask) are ranked; the others occupy no position.

  position  r_i = #{ j in the list, taking part, j != i : s_j > s_i or (s_j == s_i and j < i) }, from 0; j < i compares original row indices,
            so ties are broken and the positions of a list form a permutation.  q_i is the same count on the labels.
  discount  D(r) = 1 / log2(2 + r), and 0 for r >= topn when topn is given
  gain      G(y) = 2**y - 1 (gain='exp2') or y (gain='linear')
  list sums DCG = sum G(y_i) D(r_i), IDCG = sum G(y_i) D(q_i);  inv = 1 / IDCG where IDCG > 0, else 0
  weight    lambda_ij = |G(y_i) - G(y_j)| * |D(r_i) - D(r_j)| * inv(list), a constant in the backward pass
  metric    NDCG of a list = DCG / IDCG; the batch metric is the mean over the lists with IDCG > 0 (0 when there is none)

Everything is computed by csrc/pairwise_lambda.hip (recnow_pair_lambda_terms): one compare-only traversal of every segment, fp64 logarithms
and list sums, no host synchronisation, bitwise reproducible."""
import collections

import torch

from .. import _lib
from ._segments import _FLAG_MEMBERS_PACKED, _inputs

_GAIN_CODE = {'exp2': 0, 'linear': 1}          # RECNOW_NDCG_GAIN_* of include/recnow.h


def _check_options(gain, topn):
    if not isinstance(gain, str) or gain not in _GAIN_CODE:
        raise ValueError("gain must be 'exp2' or 'linear', got %r" % (gain,))
    if topn is not None and (isinstance(topn, bool) or not isinstance(topn, int) or topn < 1 or topn > 2 ** 31 - 1):
        raise ValueError('topn must be None or a positive integer, got %r' % (topn,))


class NDCGLambdaWeight(object):
    """The pair weight |delta NDCG| of LambdaRank as `lambda_weight=` of `pairwise_loss` / `pairwise_loss_fused`: how much the list's NDCG would
    change if the two rows of a pair swapped their places in the list ranked by the current scores.  An immutable description; the weight itself
    needs the scores and the list, so it cannot be a `label_pair_to_weight_func`.  gain: 'exp2' (2**y - 1) or 'linear' (y); topn: None, or the
    number of leading positions that carry a discount."""

    __slots__ = ('gain', 'topn')

    def __init__(self, gain='exp2', topn=None):
        _check_options(gain, topn)
        object.__setattr__(self, 'gain', gain)
        object.__setattr__(self, 'topn', topn)

    def __setattr__(self, name, value):
        raise AttributeError('NDCGLambdaWeight is immutable')

    def __delattr__(self, name):
        raise AttributeError('NDCGLambdaWeight is immutable')

    def __eq__(self, other):
        return isinstance(other, NDCGLambdaWeight) and (self.gain, self.topn) == (other.gain, other.topn)

    def __hash__(self):
        return hash((self.gain, self.topn))

    def __repr__(self):
        return 'NDCGLambdaWeight(gain=%r, topn=%r)' % (self.gain, self.topn)


NDCGRankTerms = collections.namedtuple('NDCGRankTerms', ['rank', 'discount', 'gain', 'inv_idcg'])


def lambda_workspace(B, device):
    """The workspace a count call, `rank_terms_packed` and the lambda walk share (recnow_pair_lambda_workspace_bytes)."""
    return _lib.workspace(_lib.load().recnow_pair_lambda_workspace_bytes(B), device)


def rank_terms_packed(seg, ws, gain, topn):
    """The pre-pass on a workspace whose members a count call has just packed: leaves the {discount, gain} records and inv in `ws` for
    recnow_pair_lambda_fwdbwd; returns nothing."""
    _lib.call('recnow_pair_lambda_terms', None, None, None, _lib.ptr(seg.order), _lib.ptr(seg.seg_id), _lib.ptr(seg.seg_first), seg.B,
              _FLAG_MEMBERS_PACKED, _GAIN_CODE[gain], int(topn or 0), None, None, None, None, None, None, None, None, _lib.ptr(ws), ws.numel(),
              _lib.stream())


def ndcg_rank_terms(outputs, labels, groups, mask=None, gain='exp2', topn=None, segments=None):
    """Per original row, as flat tensors of B elements: `rank` (int32 position inside the row's list, -1 for a row that does not take part),
    `discount` D(rank), `gain` G(label) and `inv_idcg` 1 / IDCG of the row's list (0 where IDCG is not positive) -- float32; discount and gain
    are 0 for a row that does not take part.  lambda_ij = |gain_i - gain_j| * |discount_i - discount_j| * inv_idcg_i for two rows of one list.
    No host synchronisation, no gradient.  segments: a precomputed `group_rows(groups)` (`groups` is then not looked at)."""
    _check_options(gain, topn)
    seg, scores, labs, m = _inputs(outputs, labels, groups, mask, segments)
    B, dev = seg.B, seg.device
    rank = torch.empty(max(B, 1), dtype=torch.int32, device=dev)
    disc, gn, inv = (torch.empty(max(B, 1), dtype=torch.float32, device=dev) for _ in range(3))
    ws = lambda_workspace(B, dev)
    _lib.call('recnow_pair_lambda_terms', _lib.ptr(scores), _lib.ptr(labs), _lib.ptr(m), _lib.ptr(seg.order), _lib.ptr(seg.seg_id),
              _lib.ptr(seg.seg_first), B, 0, _GAIN_CODE[gain], int(topn or 0), _lib.ptr(rank), _lib.ptr(disc), _lib.ptr(gn), _lib.ptr(inv), None,
              None, None, None, _lib.ptr(ws), ws.numel(), _lib.stream())
    return NDCGRankTerms(rank[:B], disc[:B], gn[:B], inv[:B])


def in_batch_ndcg(outputs, labels, groups, mask=None, gain='exp2', topn=None, segments=None):
    """(mean NDCG over the lists whose IDCG is positive -- 0 when there is none --, number of such lists) as 0-dim tensors (float32, int64).
    No host synchronisation, no gradient."""
    _check_options(gain, topn)
    seg, scores, labs, m = _inputs(outputs, labels, groups, mask, segments)
    B, dev = seg.B, seg.device
    mean = torch.empty((), dtype=torch.float32, device=dev)
    n_lists = torch.empty((), dtype=torch.int64, device=dev)
    ws = lambda_workspace(B, dev)
    _lib.call('recnow_pair_lambda_terms', _lib.ptr(scores), _lib.ptr(labs), _lib.ptr(m), _lib.ptr(seg.order), _lib.ptr(seg.seg_id),
              _lib.ptr(seg.seg_first), B, 0, _GAIN_CODE[gain], int(topn or 0), None, None, None, None, None, None, _lib.ptr(mean),
              _lib.ptr(n_lists), _lib.ptr(ws), ws.numel(), _lib.stream())
    return mean, n_lists
