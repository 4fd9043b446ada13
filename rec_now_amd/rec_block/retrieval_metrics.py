"""In-batch retrieval metrics: the ranks of the positives under the logits of the in-batch sampled softmax, and recall@K, NDCG@K, MRR and the
mean rank made of them.  An addition; the reference has no such metric.

Taking part, candidates C(i) and logits s_ij are those of rec_block/in_batch_softmax.py, extras included.  Every metric here is a function
of ONE integer per row: how many candidates score above the positive.  With `pos = s_ii` and `C'(i) = C(i) \\ {i}`, for a taking-part row

  n_candidates[i] = |C'(i)|
  n_greater[i]    = #{j in C'(i): not (s_ij <= pos)}      a NaN logit, or a NaN pos, counts as greater: a broken model must not look good
  n_equal[i]      = #{j in C'(i): s_ij == pos}

and 0, 0, 0 (with a NaN `row_pos_logit`) for a row that does not take part; such rows and masked extras may hold anything, NaN included.

Candidate mode.  `in_batch_candidates=True`: the candidates of the loss.  `False`: full-corpus evaluation -- batch item i is row i's positive
and nothing else; no batch column is a candidate of any row, the candidates are the extras alone (`extra_item` is the corpus, with its mask
and the id-hit rule: the corpus' own copy of the label is removed by id).

No (B, B + N) tensor exists at any time: one launch of the loss's kernel template (csrc/in_batch_softmax.hip, MODE 3) forms the logit tiles
on chip and keeps three integers per lane.  The positive's logit and every candidate's are results of one fp32 expression on one MFMA
chain, so a candidate that is a bit-identical copy of the positive is counted equal wherever it stands, and `row_pos_logit` is the
`row_pos_logit` of `in_batch_softmax_terms` bit for bit.  No atomics, no workspace, no host synchronisation; bitwise reproducible.

Ties.  With g = n_greater and e = n_equal the positive's rank r is g + 1 ('optimistic'), g + e + 1 ('pessimistic'), or uniform on
g + 1 .. g + e + 1 ('expected': random tie-breaking, Sun et al. 2020, "A Re-evaluation of Knowledge Graph Completion Methods").  'expected'
is the default: a collapsed tower whose logits are all equal must not score recall 1.  The expectation is exact: every per-row quantity
f(r) is summed over the tie range through an fp64 prefix-sum table over r = 1 .. B + N + 1 (sized by shapes alone), gathered at g and
g + e + 1."""
import collections
import numbers

import torch

from .. import _lib
from .in_batch_softmax import _check, _check_extra, _prepare, _prepare_extra

InBatchRanks = collections.namedtuple('InBatchRanks', ['n_greater', 'n_equal', 'n_candidates', 'row_pos_logit', 'n_rows'])
InBatchRetrievalMetrics = collections.namedtuple('InBatchRetrievalMetrics', ['recall', 'ndcg', 'mrr', 'mean_rank', 'n_rows'])

TIES = ('expected', 'optimistic', 'pessimistic')


def _ranks(query, item, item_ids, log_q, temperature, mask, remove_accidental_hits, extra_item, extra_item_ids, extra_log_q, extra_mask,
           in_batch_candidates):
    """(InBatchRanks, on): on is the (B,) bool vector of the taking-part rows, or None when every row takes part."""
    B, D = _check(query, item, item_ids, log_q, temperature, mask)
    _check_extra(query, item_ids, log_q, extra_item, extra_item_ids, extra_log_q, extra_mask)
    if not in_batch_candidates and extra_item is None:
        raise ValueError('in_batch_candidates=False scores the batch against a corpus: extra_item is required')
    dev = query.device
    if B == 0:
        z = torch.zeros(0, dtype=torch.int64, device=dev)
        return InBatchRanks(z, z.clone(), z.clone(), torch.empty(0, dtype=torch.float32, device=dev),
                            torch.zeros((), dtype=torch.int64, device=dev)), None
    q, v, ids, lq, m, B = _prepare(query, item, item_ids, log_q, mask)
    e, eids, elq, em = _prepare_extra(extra_item, extra_item_ids, extra_log_q, extra_mask)
    counts = torch.empty((3, B), dtype=torch.int64, device=dev)
    pos = torch.empty(B, dtype=torch.float32, device=dev)
    P = _lib.ptr
    _lib.call('recnow_ibs_rank', P(q), q.stride(0), P(v), v.stride(0), P(ids), P(lq), P(m), B, D, P(e), 0 if e is None else e.stride(0),
              P(eids), P(elq), P(em), 0 if e is None else e.shape[0], 1.0 / float(temperature), 1 if remove_accidental_hits else 0,
              1 if in_batch_candidates else 0, P(counts[0]), P(counts[1]), P(counts[2]), P(pos), _lib.stream())
    n_rows = torch.full((), B, dtype=torch.int64, device=dev) if m is None else m.sum(dtype=torch.int64)
    return InBatchRanks(counts[0], counts[1], counts[2], pos, n_rows), (None if m is None else m != 0)


def in_batch_ranks(query, item, item_ids=None, log_q=None, temperature=1.0, mask=None, remove_accidental_hits=True, *, extra_item=None,
                   extra_item_ids=None, extra_log_q=None, extra_mask=None, in_batch_candidates=True):
    """The counts every retrieval metric is made of (module docstring); arguments as in_batch_softmax_loss, (B, D) float32 GPU tensors,
    D <= 128.  Returns InBatchRanks(n_greater, n_equal, n_candidates, row_pos_logit, n_rows):
      n_greater, n_equal, n_candidates (B,) int64    0 where the row does not take part
      row_pos_logit (B,) float32                     s_ii; NaN where the row does not take part
      n_rows () int64                                the number of taking-part rows
    No gradient, no host synchronisation; one launch."""
    return _ranks(query, item, item_ids, log_q, temperature, mask, remove_accidental_hits, extra_item, extra_item_ids, extra_log_q, extra_mask,
                  in_batch_candidates)[0]


def _check_k(k, ties):
    if ties not in TIES:
        raise ValueError('ties must be one of %s, got %r' % (TIES, ties))
    if isinstance(k, numbers.Integral) and not isinstance(k, bool):
        k = (k,)
    try:
        k = tuple(k)
    except TypeError:
        raise ValueError('k must be a positive int or a sequence of them, got %r' % (k,))
    if len(k) == 0:
        raise ValueError('k must name at least one K')
    for kk in k:
        if isinstance(kk, bool) or not isinstance(kk, numbers.Integral) or kk <= 0:
            raise ValueError('every K must be a positive int, got %r' % (kk,))
    return tuple(int(kk) for kk in k)


_TABLES = {}


def _tables(M, dev):
    """fp64 prefix sums over r = 1 .. M of 1 / log2(1 + r) and 1 / r, entry 0 = 0: (2, M + 1).  Kept per (device, M), except while a graph is
    being captured (what is allocated then belongs to the graph)."""
    key = (dev.type, dev.index, M)
    hit = _TABLES.get(key)
    if hit is not None:
        return hit
    r = torch.arange(0, M + 1, dtype=torch.float64, device=dev)
    t = torch.stack([1.0 / torch.log2(1.0 + r), 1.0 / r])
    t[:, 0] = 0.0
    t = torch.cumsum(t, dim=1)
    if not (dev.type == 'cuda' and torch.cuda.is_current_stream_capturing()):
        if len(_TABLES) >= 16:
            _TABLES.clear()
        _TABLES[key] = t
    return t


def metrics_from_counts(n_greater, n_equal, on, n_rows, n_ranks, k=(1, 10, 100), ties='expected'):
    """The aggregation of in_batch_retrieval_metrics on given counts: (B,) integer n_greater / n_equal, `on` (B,) bool or None (every row
    takes part), n_rows 0-dim, n_ranks >= max(n_greater + n_equal) + 1 (the table's length; B + N + 1 from shapes).  Torch on (B,) vectors,
    on the device of the counts."""
    k = _check_k(k, ties)
    dev = n_greater.device
    g, e = n_greater.to(torch.int64), n_equal.to(torch.int64)
    # the rank is uniform on lo + 1 .. hi
    lo = g + e if ties == 'pessimistic' else g
    hi = g + 1 if ties == 'optimistic' else g + e + 1
    width = (hi - lo).to(torch.float64)
    tab = _tables(int(n_ranks), dev)
    w = torch.ones_like(width) if on is None else on.to(torch.float64)
    n = n_rows.to(torch.float64)
    w = w / torch.clamp(n, min=1.0)                    # the mean over the taking-part rows
    wt = w / width                                     # ... and over the tie range at once
    recall, ndcg = [], []
    for kk in k:                                       # ranks above K add nothing: both ends of the range are cut at K
        hi_k, lo_k = hi.clamp(max=kk), lo.clamp(max=kk)
        recall.append(((hi_k - lo_k).to(torch.float64) * wt).sum())                    # the prefix sum of [r <= K] is min(r, K)
        ndcg.append(((tab[0][hi_k] - tab[0][lo_k]) * wt).sum())
    mrr = ((tab[1][hi] - tab[1][lo]) * wt).sum()
    mean_rank = ((lo + hi + 1).to(torch.float64) * 0.5 * w).sum()                      # the mean of lo + 1 .. hi, exact in integers
    return InBatchRetrievalMetrics(torch.stack(recall), torch.stack(ndcg), mrr, mean_rank, n_rows)


def in_batch_retrieval_metrics(query, item, item_ids=None, log_q=None, temperature=1.0, mask=None, remove_accidental_hits=True, *,
                               extra_item=None, extra_item_ids=None, extra_log_q=None, extra_mask=None, in_batch_candidates=True,
                               k=(1, 10, 100), ties='expected'):
    """recall@K, NDCG@K, MRR and the mean rank of the positives (module docstring), means over the taking-part rows (0 when there are none)
    of [r <= K], [r <= K] / log2(1 + r), 1 / r and r.  k: positive ints;  ties: 'expected' (default), 'optimistic' or 'pessimistic'.
    Returns InBatchRetrievalMetrics(recall, ndcg (len(k),) float64 in the order of k;  mrr, mean_rank () float64;  n_rows () int64).
    The hot path is the count launch of in_batch_ranks; the rest is torch on (B,) vectors.  No host synchronisation."""
    k = _check_k(k, ties)
    ranks, on = _ranks(query, item, item_ids, log_q, temperature, mask, remove_accidental_hits, extra_item, extra_item_ids, extra_log_q,
                       extra_mask, in_batch_candidates)
    B = query.shape[0]
    dev = query.device
    if B == 0:
        z = torch.zeros(len(k), dtype=torch.float64, device=dev)
        s = torch.zeros((), dtype=torch.float64, device=dev)
        return InBatchRetrievalMetrics(z, z.clone(), s, s.clone(), ranks.n_rows)
    N = 0 if extra_item is None else extra_item.shape[0]
    return metrics_from_counts(ranks.n_greater, ranks.n_equal, on, ranks.n_rows, B + N + 1, k, ties)
