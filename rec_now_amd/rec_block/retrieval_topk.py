"""In-batch top-K candidates: for every row, the K candidates that score highest under the logits of the in-batch sampled softmax.  That
is hard-negative mining (a row's K hardest negatives from the batch, a memory bank or the gathered items of other ranks) and top-K retrieval
of a corpus.  An addition; the reference has no such operation.

Taking part, the candidates C'(i) = C(i) \\ {i}, the logits s_ij and `in_batch_candidates=False` (the candidates are the extras alone,
`extra_item` is the corpus) are exactly those of rec_block/retrieval_metrics.py.  The positive is never in the list.

Indices address `cat(item, extra_item)` in both candidate modes: batch column j is j, extra k is B + k.

Order.  Candidate a stands before candidate b iff a's score is NaN and b's is not, or score_a > score_b, or the scores compare equal (or
both are NaN) and index_a < index_b.  The order is total, so the result is a function of the candidate set alone; -0.0 and 0.0 tie, and NaN
is greatest, as in torch.topk and as `n_greater` counts it.

Row i holds the first min(k, |C'(i)|) candidates in that order; the remaining slots are filled with score -inf and index -1.  A candidate
whose logit is -inf is a candidate: it carries its index and stands before the fill.  Rows that do not take part get all fill and
n_candidates 0; such rows and masked extras may hold anything, NaN included.

No (B, B + N) tensor exists at any time: one launch of the loss's kernel template (csrc/in_batch_softmax.hip, MODE 4) forms the logit
tiles on chip and keeps each row's list in LDS.  A returned score is the result of the one fp32 expression `in_batch_ranks` compares and
`in_batch_softmax_terms` exponentiates.  No atomics, no workspace, no host synchronisation; bitwise reproducible."""
import collections
import numbers

import torch

from .. import _lib
from .in_batch_softmax import _check, _check_extra, _prepare, _prepare_extra

InBatchTopK = collections.namedtuple('InBatchTopK', ['scores', 'indices', 'n_candidates'])


MAX_K = 128                                     # recnow_ibs_topk_max_k(): 64 rows of K (score, index) slots in LDS beside the tile


def in_batch_top_k(query, item, item_ids=None, log_q=None, temperature=1.0, mask=None, remove_accidental_hits=True, *, k, extra_item=None,
                   extra_item_ids=None, extra_log_q=None, extra_mask=None, in_batch_candidates=True):
    """The k highest-scoring candidates of every row (module docstring); arguments as in_batch_ranks, (B, D) float32 GPU tensors, D <= 128;
    k: a positive int, at most MAX_K.  Returns InBatchTopK(scores, indices, n_candidates):
      scores (B, k) float32     descending in the total order; -inf in the slots past the row's candidates
      indices (B, k) int64      into cat(item, extra_item); -1 in those slots
      n_candidates (B,) int64   |C'(i)|; 0 where the row does not take part
    No gradient, no host synchronisation; one launch."""
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k <= 0:
        raise ValueError('k must be a positive int, got %r' % (k,))
    k = int(k)
    B, D = _check(query, item, item_ids, log_q, temperature, mask)
    _check_extra(query, item_ids, log_q, extra_item, extra_item_ids, extra_log_q, extra_mask)
    if not in_batch_candidates and extra_item is None:
        raise ValueError('in_batch_candidates=False scores the batch against a corpus: extra_item is required')
    dev = query.device
    if k > MAX_K:
        raise NotImplementedError('in_batch_top_k keeps at most %d candidates a row, got k = %d' % (MAX_K, k))
    if B == 0:
        return InBatchTopK(torch.empty((0, k), dtype=torch.float32, device=dev), torch.empty((0, k), dtype=torch.int64, device=dev),
                           torch.zeros(0, dtype=torch.int64, device=dev))
    q, v, ids, lq, m, B = _prepare(query, item, item_ids, log_q, mask)
    e, eids, elq, em = _prepare_extra(extra_item, extra_item_ids, extra_log_q, extra_mask)
    scores = torch.empty((B, k), dtype=torch.float32, device=dev)
    indices = torch.empty((B, k), dtype=torch.int64, device=dev)
    n_cand = torch.empty(B, dtype=torch.int64, device=dev)
    P = _lib.ptr
    _lib.call('recnow_ibs_topk', P(q), q.stride(0), P(v), v.stride(0), P(ids), P(lq), P(m), B, D, P(e), 0 if e is None else e.stride(0),
              P(eids), P(elq), P(em), 0 if e is None else e.shape[0], 1.0 / float(temperature), 1 if remove_accidental_hits else 0,
              1 if in_batch_candidates else 0, k, P(scores), k, P(indices), k, P(n_cand), _lib.stream())
    return InBatchTopK(scores, indices, n_cand)
