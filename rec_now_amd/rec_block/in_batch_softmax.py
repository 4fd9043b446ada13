"""In-batch sampled softmax: the retrieval loss two-tower models train on.  Row i's query embedding is scored against the item embedding of
EVERY row of the batch; the item of row i is the positive, all the others are negatives.  An addition; the reference has no such loss.

Logit.  `s_ij = <query_i, item_j> / temperature - log_q[j]` -- the logQ correction of Yi et al. 2019 ("Sampling-bias-corrected neural
modeling"), applied to every column, the positive included.  `log_q` carries no gradient.

Taking part.  Row i takes part iff `mask` is None or non-zero there.

Candidates.  Column j is a candidate of row i iff `j == i`, or `mask_j != 0` and not (`remove_accidental_hits` and `item_ids` given and
`item_ids[j] == item_ids[i]`) -- the accidental-hit removal of the TF-Recommenders Retrieval task.

Loss.  `l_i = lse_{j in C(i)} s_ij - s_ii`; returned is the mean over the taking-part rows (0 when there are none) as a 0-dim float32 tensor,
without a host synchronisation: the call can be captured in a HIP graph.

Gradient.  With n taking-part rows and `p_ij = exp(s_ij - lse_i)` on candidates, 0 elsewhere:
`dq_i = 1 / (n tau) sum_j (p_ij - [j == i]) item_j`, `dv_j = 1 / (n tau) sum_i (p_ij - [j == i]) query_i` over the taking-part i.  Rows that
do not take part get 0 and may hold anything, NaN included; a NaN in a taking-part row makes the loss NaN (every row sees every item).

No (B, B) tensor exists at any time: the logit tiles are formed on chip (exact fp32 MFMA), the forward keeps two floats per row, the backward
recomputes the tiles (csrc/in_batch_softmax.hip).  No atomics, bitwise reproducible.  A row whose only candidate is itself has loss exactly 0
and contributes exactly zero gradient.  `query` / `item` may be row-strided views (a column slice of a wider tower output): no copy.

Extra negatives.  `extra_item` (N, D) adds N rows on the item side that have no query row of their own: uniformly sampled items put through
the item tower beside the batch (mixed negative sampling, Yang et al. 2020), a bank of earlier steps' item embeddings (cross-batch negatives,
Wang et al. 2021; pass it detached), or the other ranks' items after an all-gather.  Extra k is a candidate of row i iff row i takes part,
`extra_mask` is None or non-zero at k, and not (`remove_accidental_hits` and ids given and `extra_item_ids[k] == item_ids[i]`); it is never
a positive.  Its logit is `s_{i,B+k} = <q_i, e_k> / tau - extra_log_q[k]`.  Everything above holds with the larger candidate set; `dq_i` gains
`1 / (n tau) sum_k p_{i,B+k} e_k`, and `de_k = 1 / (n tau) sum_i p_{i,B+k} q_i` over the taking-part rows.  An extra whose mask is 0 may hold
anything, NaN included, and gets 0.  No (B, B + N) tensor exists either: the extras go through the same on-chip tile after the items, and
no tensor but `de` is sized by N x D (the per-extra vectors are held as the kernels read them -- int64 ids, fp32 `extra_log_q`, a uint8 mask,
at most 13 N bytes where a conversion was needed); when `extra_item` does not require grad, `de` is not computed."""
import collections
import math
import numbers

import torch

from .. import _lib

MAX_D = 128

InBatchSoftmaxTerms = collections.namedtuple('InBatchSoftmaxTerms', ['row_lse', 'row_pos_logit', 'row_loss', 'n_rows'])


def _check(query, item, item_ids, log_q, temperature, mask):
    """The argument errors that need no device.  Returns (B, D)."""
    for t, what in ((query, 'query'), (item, 'item')):
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s must be a torch.Tensor, got %s' % (what, type(t)))
        if t.dim() != 2:
            raise ValueError('%s must be of rank 2 (B, D), got shape %s' % (what, tuple(t.shape)))
    if query.shape != item.shape:
        raise ValueError('query and item must have the same shape: %s and %s' % (tuple(query.shape), tuple(item.shape)))
    B, D = query.shape
    for t, what in ((item_ids, 'item_ids'), (log_q, 'log_q'), (mask, 'mask')):
        if t is not None and t.numel() != B:
            raise ValueError('%s must have one element per row: %d elements for %d rows' % (what, t.numel(), B))
    if item_ids is not None and (item_ids.is_floating_point() or item_ids.is_complex() or item_ids.dtype == torch.bool):
        raise ValueError('item_ids must be an integer tensor, got %s' % item_ids.dtype)
    if isinstance(temperature, bool) or not isinstance(temperature, numbers.Real) or not math.isfinite(temperature) or temperature <= 0:
        raise ValueError('temperature must be a finite number > 0, got %r' % (temperature,))
    if D > MAX_D:
        raise NotImplementedError('in_batch_softmax: D = %d; the fused kernels hold a row on chip up to D = %d' % (D, MAX_D))
    return B, D


def _check_extra(query, item_ids, log_q, extra_item, extra_item_ids, extra_log_q, extra_mask):
    """The argument errors of the extra negatives.  Returns N, or None without extras."""
    if extra_item is None:
        for t, what in ((extra_item_ids, 'extra_item_ids'), (extra_log_q, 'extra_log_q'), (extra_mask, 'extra_mask')):
            if t is not None:
                raise ValueError('%s given without extra_item' % what)
        return None
    if not isinstance(extra_item, torch.Tensor):
        raise TypeError('extra_item must be a torch.Tensor, got %s' % type(extra_item))
    if extra_item.dim() != 2:
        raise ValueError('extra_item must be of rank 2 (N, D), got shape %s' % (tuple(extra_item.shape),))
    N, D = extra_item.shape
    if D != query.shape[1]:
        raise ValueError('extra_item must have the D of query: %d and %d' % (D, query.shape[1]))
    if extra_item.device != query.device:
        raise ValueError('extra_item must be on the device of query: %s and %s' % (extra_item.device, query.device))
    for t, what in ((extra_item_ids, 'extra_item_ids'), (extra_log_q, 'extra_log_q'), (extra_mask, 'extra_mask')):
        if t is not None and t.numel() != N:
            raise ValueError('%s must have one element per extra: %d elements for %d extras' % (what, t.numel(), N))
    if extra_item_ids is not None and (extra_item_ids.is_floating_point() or extra_item_ids.is_complex() or extra_item_ids.dtype == torch.bool):
        raise ValueError('extra_item_ids must be an integer tensor, got %s' % extra_item_ids.dtype)
    if (extra_item_ids is None) != (item_ids is None):
        raise ValueError('item_ids and extra_item_ids go together: an accidental hit is an equal pair of them')
    if (extra_log_q is None) != (log_q is None):      # a correction on one side only is a bias between the two candidate sets
        raise ValueError('log_q and extra_log_q go together: a logQ correction of one candidate set alone is a bias')
    return N


def _rows(t, what):
    """fp32 rows the kernels can walk: unit column stride, any row stride >= D (no copy for a column slice of a wider tensor)."""
    _lib.require_gpu(t, what)
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def _prepare(query, item, item_ids, log_q, mask):
    q, v = _rows(query, 'query'), _rows(item, 'item')
    B = q.shape[0]
    ids = lq = m = None
    if item_ids is not None:
        ids = _lib.require_gpu(item_ids, 'item_ids').detach().reshape(-1).to(torch.int64).contiguous()
    if log_q is not None:
        lq = _lib.f32c(log_q, 'log_q').detach().reshape(-1)
    if mask is not None:
        m = (_lib.require_gpu(mask, 'mask').detach().reshape(-1) != 0).to(torch.uint8).contiguous()
    return q, v, ids, lq, m, B


def _prepare_extra(extra_item, extra_item_ids, extra_log_q, extra_mask):
    """(e, eids, elq, em) for the library; all None without extras or with N = 0 (the square entries run)."""
    if extra_item is None or extra_item.shape[0] == 0:
        return None, None, None, None
    e = _rows(extra_item, 'extra_item')
    eids = elq = em = None
    if extra_item_ids is not None:
        eids = _lib.require_gpu(extra_item_ids, 'extra_item_ids').detach().reshape(-1).to(torch.int64).contiguous()
    if extra_log_q is not None:
        elq = _lib.f32c(extra_log_q, 'extra_log_q').detach().reshape(-1)
    if extra_mask is not None:
        em = (_lib.require_gpu(extra_mask, 'extra_mask').detach().reshape(-1) != 0).to(torch.uint8).contiguous()
    return e, eids, elq, em


def _forward(q, v, ids, lq, m, temperature, remove, e=None, eids=None, elq=None, em=None):
    B, D = q.shape
    dev = q.device
    stat = torch.empty((4, B), dtype=torch.float32, device=dev)          # row_max, row_logsum, row_pos, row_loss
    out = torch.empty(2, dtype=torch.float32, device=dev)                # loss, n_rows
    ws = _lib.workspace(_lib.load().recnow_ibs_workspace_bytes(B, D, 0), dev)
    P = _lib.ptr
    if e is None:
        _lib.call('recnow_ibs_fwd', P(q), q.stride(0), P(v), v.stride(0), P(ids), P(lq), P(m), B, D, 1.0 / float(temperature),
                  1 if remove else 0, P(stat[0]), P(stat[1]), P(stat[2]), P(stat[3]), P(out[0:]), P(out[1:]), P(ws), ws.numel(), _lib.stream())
    else:
        _lib.call('recnow_ibs_extra_fwd', P(q), q.stride(0), P(v), v.stride(0), P(ids), P(lq), P(m), B, D, P(e), e.stride(0), P(eids), P(elq),
                  P(em), e.shape[0], 1.0 / float(temperature), 1 if remove else 0, P(stat[0]), P(stat[1]), P(stat[2]), P(stat[3]),
                  P(out[0:]), P(out[1:]), P(ws), ws.numel(), _lib.stream())
    return stat, out


class _InBatchSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, query, item, item_ids, log_q, mask, temperature, remove, extra_item, extra_item_ids, extra_log_q, extra_mask):
        q, v, ids, lq, m, B = _prepare(query, item, item_ids, log_q, mask)
        e, eids, elq, em = _prepare_extra(extra_item, extra_item_ids, extra_log_q, extra_mask)
        stat, out = _forward(q, v, ids, lq, m, temperature, remove, e, eids, elq, em)
        ctx.temperature, ctx.remove = float(temperature), bool(remove)
        ctx.q_dtype, ctx.v_dtype = query.dtype, item.dtype
        ctx.e_dtype, ctx.e_shape = (None, None) if extra_item is None else (extra_item.dtype, tuple(extra_item.shape))
        ctx.save_for_backward(q, v, ids, lq, m, stat, out, e, eids, elq, em)
        loss, n_rows = out[0], out[1]
        ctx.mark_non_differentiable(n_rows)
        return loss, n_rows

    @staticmethod
    def backward(ctx, g, _gn):
        q, v, ids, lq, m, stat, out, e, eids, elq, em = ctx.saved_tensors
        B, D = q.shape
        dev = q.device
        want_q, want_v, want_e = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[7]
        dq = torch.empty((B, D), dtype=torch.float32, device=dev) if want_q else None
        dv = torch.empty((B, D), dtype=torch.float32, device=dev) if want_v else None
        de = torch.empty(ctx.e_shape, dtype=torch.float32, device=dev) if want_e else None          # N = 0: the empty (0, D) gradient
        if want_q or want_v or (want_e and e is not None):
            g32 = g.detach().to(torch.float32).reshape(1).contiguous()
            P = _lib.ptr
            if e is None:
                _lib.call('recnow_ibs_bwd', P(q), q.stride(0), P(v), v.stride(0), P(ids), P(lq), P(m), B, D, 1.0 / ctx.temperature,
                          1 if ctx.remove else 0, P(stat[0]), P(stat[1]), P(out[1:]), P(g32), P(dq), D, P(dv), D, None, 0, _lib.stream())
            else:
                _lib.call('recnow_ibs_extra_bwd', P(q), q.stride(0), P(v), v.stride(0), P(ids), P(lq), P(m), B, D, P(e), e.stride(0), P(eids),
                          P(elq), P(em), e.shape[0], 1.0 / ctx.temperature, 1 if ctx.remove else 0, P(stat[0]), P(stat[1]), P(out[1:]),
                          P(g32), P(dq), D, P(dv), D, P(de), D, None, 0, _lib.stream())
            if want_q and ctx.q_dtype != torch.float32:
                dq = dq.to(ctx.q_dtype)
            if want_v and ctx.v_dtype != torch.float32:
                dv = dv.to(ctx.v_dtype)
        if want_e and ctx.e_dtype != torch.float32:
            de = de.to(ctx.e_dtype)
        return dq, dv, None, None, None, None, None, de, None, None, None


def in_batch_softmax_loss(query, item, item_ids=None, log_q=None, temperature=1.0, mask=None, remove_accidental_hits=True,
                          return_num_rows=False, *, extra_item=None, extra_item_ids=None, extra_log_q=None, extra_mask=None):
    """The in-batch sampled-softmax loss (module docstring), differentiable in `query` and `item` ((B, D) float32 GPU tensors, D <= 128).
    item_ids: (B,) or (B, 1) int32 / int64;  log_q: (B,) or (B, 1) float;  mask: (B,) bool or number, non-zero = the row takes part.
    extra_item: (N, D) extra negatives (module docstring), differentiable;  extra_item_ids: (N,) or (N, 1) integers, given iff item_ids is;
    extra_log_q: (N,) or (N, 1) float, given iff log_q is;  extra_mask: (N,), non-zero = the extra is a candidate (a bank not yet full).
    Returns the 0-dim float32 loss [, the number of taking-part rows as a float32 tensor]."""
    B, D = _check(query, item, item_ids, log_q, temperature, mask)
    N = _check_extra(query, item_ids, log_q, extra_item, extra_item_ids, extra_log_q, extra_mask)
    if B == 0:                                   # no row: loss 0, empty gradients (zeros for the extras), no call into the library
        loss = (query.sum() + item.sum()).to(torch.float32) * 0.0
        if N is not None:
            loss = loss + extra_item[:0].sum().to(torch.float32)
        return (loss, torch.zeros((), dtype=torch.float32, device=query.device)) if return_num_rows else loss
    for t, what in ((query, 'query'), (item, 'item')) + (() if N is None else ((extra_item, 'extra_item'),)):
        _lib.require_gpu(t, what)
    loss, n_rows = _InBatchSoftmax.apply(query, item, item_ids, log_q, mask, temperature, bool(remove_accidental_hits), extra_item,
                                         extra_item_ids, extra_log_q, extra_mask)
    return (loss, n_rows) if return_num_rows else loss


def in_batch_softmax_terms(query, item, item_ids=None, log_q=None, temperature=1.0, mask=None, remove_accidental_hits=True, *,
                           extra_item=None, extra_item_ids=None, extra_log_q=None, extra_mask=None):
    """What the loss is made of, InBatchSoftmaxTerms(row_lse, row_pos_logit, row_loss, n_rows):
      row_lse (B,) float64        lse_{j in C(i)} s_ij as the kernels keep it, maximum + log of the rescaled sum (added in fp64: nothing of
                                  the second word is lost to a large maximum); NaN where the row does not take part
      row_pos_logit (B,) float32  s_ii; NaN where the row does not take part
      row_loss (B,) float32       l_i; 0 where the row does not take part
      n_rows () float32           the number of taking-part rows
    No gradient, no host synchronisation."""
    B, D = _check(query, item, item_ids, log_q, temperature, mask)
    _check_extra(query, item_ids, log_q, extra_item, extra_item_ids, extra_log_q, extra_mask)
    if B == 0:
        dev = query.device
        return InBatchSoftmaxTerms(torch.empty(0, dtype=torch.float64, device=dev), torch.empty(0, dtype=torch.float32, device=dev),
                                   torch.empty(0, dtype=torch.float32, device=dev), torch.zeros((), dtype=torch.float32, device=dev))
    q, v, ids, lq, m, B = _prepare(query, item, item_ids, log_q, mask)
    stat, out = _forward(q, v, ids, lq, m, temperature, bool(remove_accidental_hits),
                         *_prepare_extra(extra_item, extra_item_ids, extra_log_q, extra_mask))
    return InBatchSoftmaxTerms(stat[0].double() + stat[1].double(), stat[2], stat[3], out[1])
