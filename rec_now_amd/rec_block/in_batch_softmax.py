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
and contributes exactly zero gradient.  `query` / `item` may be row-strided views (a column slice of a wider tower output): no copy."""
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


def _forward(q, v, ids, lq, m, temperature, remove):
    B, D = q.shape
    dev = q.device
    stat = torch.empty((4, B), dtype=torch.float32, device=dev)          # row_max, row_logsum, row_pos, row_loss
    out = torch.empty(2, dtype=torch.float32, device=dev)                # loss, n_rows
    ws = _lib.workspace(_lib.load().recnow_ibs_workspace_bytes(B, D, 0), dev)
    P = _lib.ptr
    _lib.call('recnow_ibs_fwd', P(q), q.stride(0), P(v), v.stride(0), P(ids), P(lq), P(m), B, D, 1.0 / float(temperature), 1 if remove else 0,
              P(stat[0]), P(stat[1]), P(stat[2]), P(stat[3]), P(out[0:]), P(out[1:]), P(ws), ws.numel(), _lib.stream())
    return stat, out


class _InBatchSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, query, item, item_ids, log_q, mask, temperature, remove):
        q, v, ids, lq, m, B = _prepare(query, item, item_ids, log_q, mask)
        stat, out = _forward(q, v, ids, lq, m, temperature, remove)
        ctx.temperature, ctx.remove = float(temperature), bool(remove)
        ctx.q_dtype, ctx.v_dtype = query.dtype, item.dtype
        ctx.save_for_backward(q, v, ids, lq, m, stat, out)
        loss, n_rows = out[0], out[1]
        ctx.mark_non_differentiable(n_rows)
        return loss, n_rows

    @staticmethod
    def backward(ctx, g, _gn):
        q, v, ids, lq, m, stat, out = ctx.saved_tensors
        B, D = q.shape
        dev = q.device
        want_q, want_v = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dq = torch.empty((B, D), dtype=torch.float32, device=dev) if want_q else None
        dv = torch.empty((B, D), dtype=torch.float32, device=dev) if want_v else None
        if want_q or want_v:
            g32 = g.detach().to(torch.float32).reshape(1).contiguous()
            P = _lib.ptr
            _lib.call('recnow_ibs_bwd', P(q), q.stride(0), P(v), v.stride(0), P(ids), P(lq), P(m), B, D, 1.0 / ctx.temperature,
                      1 if ctx.remove else 0, P(stat[0]), P(stat[1]), P(out[1:]), P(g32), P(dq), D, P(dv), D, None, 0, _lib.stream())
            if want_q and ctx.q_dtype != torch.float32:
                dq = dq.to(ctx.q_dtype)
            if want_v and ctx.v_dtype != torch.float32:
                dv = dv.to(ctx.v_dtype)
        return dq, dv, None, None, None, None, None


def in_batch_softmax_loss(query, item, item_ids=None, log_q=None, temperature=1.0, mask=None, remove_accidental_hits=True,
                          return_num_rows=False):
    """The in-batch sampled-softmax loss (module docstring), differentiable in `query` and `item` ((B, D) float32 GPU tensors, D <= 128).
    item_ids: (B,) or (B, 1) int32 / int64;  log_q: (B,) or (B, 1) float;  mask: (B,) bool or number, non-zero = the row takes part.
    Returns the 0-dim float32 loss [, the number of taking-part rows as a float32 tensor]."""
    B, D = _check(query, item, item_ids, log_q, temperature, mask)
    if B == 0:                                   # no row: loss 0, empty gradients, no call into the library
        loss = (query.sum() + item.sum()).to(torch.float32) * 0.0
        return (loss, torch.zeros((), dtype=torch.float32, device=query.device)) if return_num_rows else loss
    for t, what in ((query, 'query'), (item, 'item')):
        _lib.require_gpu(t, what)
    loss, n_rows = _InBatchSoftmax.apply(query, item, item_ids, log_q, mask, temperature, bool(remove_accidental_hits))
    return (loss, n_rows) if return_num_rows else loss


def in_batch_softmax_terms(query, item, item_ids=None, log_q=None, temperature=1.0, mask=None, remove_accidental_hits=True):
    """What the loss is made of, InBatchSoftmaxTerms(row_lse, row_pos_logit, row_loss, n_rows):
      row_lse (B,) float64        lse_{j in C(i)} s_ij as the kernels keep it, maximum + log of the rescaled sum (added in fp64: nothing of
                                  the second word is lost to a large maximum); NaN where the row does not take part
      row_pos_logit (B,) float32  s_ii; NaN where the row does not take part
      row_loss (B,) float32       l_i; 0 where the row does not take part
      n_rows () float32           the number of taking-part rows
    No gradient, no host synchronisation."""
    B, D = _check(query, item, item_ids, log_q, temperature, mask)
    if B == 0:
        dev = query.device
        return InBatchSoftmaxTerms(torch.empty(0, dtype=torch.float64, device=dev), torch.empty(0, dtype=torch.float32, device=dev),
                                   torch.empty(0, dtype=torch.float32, device=dev), torch.zeros((), dtype=torch.float32, device=dev))
    q, v, ids, lq, m, B = _prepare(query, item, item_ids, log_q, mask)
    stat, out = _forward(q, v, ids, lq, m, temperature, bool(remove_accidental_hits))
    return InBatchSoftmaxTerms(stat[0].double() + stat[1].double(), stat[2], stat[3], out[1])
