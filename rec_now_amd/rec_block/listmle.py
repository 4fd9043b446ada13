"""In-batch ListMLE: the negative log-likelihood of the label-sorted permutation of every list under the Plackett-Luce model.  An addition
beside the softmax loss of `listwise_loss_from_batch` (which treats a list as a bag); the reference has no ListMLE.

Lists.  Those of `listwise_loss_from_batch`: `build_segments(group_ids, inf_equal=True)` (tf.unique equality; a list of id tensors means
agreement in every one), numbered by first occurrence in the batch.

Taking part.  A row takes part if `mask` is None or non-zero there, and its label is not NaN.  Other rows get gradient 0 and influence nothing.

Permutation.  The taking-part rows of a list by label descending (-0.0 and +0.0 are one value), ties by ascending original row index
(deterministic; TF-Ranking breaks ties at random).  `n` is their number, `s_1 .. s_n` their logits in that order.

Valid list.  `n >= 2` and at least two distinct label values among the taking-part rows.

Loss of a list.  With `K = n` if `topn is None`, else `min(topn, n)`:  `l = sum_{p=1..K} (lse_p - s_p)`, `lse_p = log sum_{q>=p} exp(s_q)`;
divided by `K` with `list_mean=True`; multiplied by `weights[rank of the list among the valid lists, first-occurrence order]`.

Gradient.  Before weight and `1/K`:  `dl/ds_q = exp(s_q + logA_q) - [q <= K]`, `logA_q = log sum_{p <= min(q,K)} exp(-lse_p)`.

Reduction.  `do_reduce=True`: the mean over the valid lists, 0 when there is none, without a host synchronisation (the call can be captured in
a HIP graph).  `do_reduce=False`: the `(n_valid,)` per-list losses in first-occurrence order, at the price of one host synchronisation.

Non-finite logits.  A non-finite logit of a taking-part row makes that list's loss non-finite and its taking-part rows' gradients NaN; nothing
else.  Where a grouping call reports a grid-barrier time-out, the loss and the gradient are NaN and the number of lists is -1.

fp64 scans, no atomics, bitwise reproducible (csrc/listmle.hip, recnow_listmle_fwdbwd)."""
import collections
import numbers

import torch

from .. import _lib
from ._segments import build_segments, _flat_mask

ListMLETerms = collections.namedtuple('ListMLETerms', ['position', 'lse', 'list_loss', 'valid'])


def _numel(t):
    if isinstance(t, (list, tuple)) and len(t) > 0 and all(isinstance(g, torch.Tensor) for g in t):
        return t[0].numel()
    return t.numel() if isinstance(t, torch.Tensor) else len(t)


def _check(group_ids, labels, logits, weights, mask, topn):
    """The argument errors that need no device."""
    if topn is not None and (isinstance(topn, bool) or not isinstance(topn, numbers.Integral) or topn < 1):
        raise ValueError('topn must be None or an integer >= 1, got %r' % (topn,))
    B = _numel(group_ids)
    for t, what in ((labels, 'labels'), (logits, 'logits'), (mask, 'mask')):
        if t is not None and t.numel() != B:
            raise ValueError('group_ids, labels, logits and mask must have the same number of elements: %d ids, %d %s' % (B, t.numel(), what))
    if isinstance(group_ids, (list, tuple)) and any(isinstance(g, torch.Tensor) and g.numel() != B for g in group_ids):
        raise ValueError('all group tensors must have the same number of elements')
    if weights is not None and weights.numel() > B:
        raise ValueError('weights must have one entry per valid list: %d weights for %d rows' % (weights.numel(), B))
    return B


def _run(group_ids, labels, logits, weights, mask, topn, list_mean, reduce, want_grad, want_terms):
    B = _check(group_ids, labels, logits, weights, mask, topn)
    for t, what in ((logits, 'logits'), (labels, 'labels')):
        _lib.require_gpu(t, what)
    seg = build_segments(group_ids.reshape(-1) if isinstance(group_ids, torch.Tensor) else group_ids, inf_equal=True)
    dev = seg.device
    lab = _lib.f32c(labels, 'labels').reshape(-1).detach()
    lg = _lib.f32c(logits, 'logits').reshape(-1).detach()
    m = _flat_mask(mask, B)
    w = None
    if weights is not None:
        w = _lib.f32c(weights, 'weights').reshape(-1).detach()
        if w.numel() < B:          # the kernel reads weights[rank of a valid list] (<= B lists): never past the buffer's end
            w = torch.cat([w, w.new_zeros(B - w.numel())])
    n = max(B, 1)
    out = {}
    if want_grad:
        out['loss'] = torch.empty((), dtype=torch.float32, device=dev)
        out['n_valid'] = torch.empty((), dtype=torch.int32, device=dev)
        out['dbase'] = torch.empty(n, dtype=torch.float32, device=dev)
        out['row_rank'] = torch.empty(n, dtype=torch.int32, device=dev)
        out['group_loss'] = torch.empty(n, dtype=torch.float32, device=dev)
    if want_terms:
        out['position'] = torch.empty(n, dtype=torch.int32, device=dev)
        out['row_lse'] = torch.empty(n, dtype=torch.float64, device=dev)
        out['list_loss'] = torch.empty(n, dtype=torch.float64, device=dev)
        out['list_valid'] = torch.empty(n, dtype=torch.int32, device=dev)
    P = _lib.ptr
    nws = _lib.load().recnow_listmle_workspace_bytes(B)
    ws = _lib.workspace(nws, dev)
    _lib.call('recnow_listmle_fwdbwd', P(lab), P(lg), P(m), P(w), P(seg.order), P(seg.seg_id), P(seg.seg_first), P(seg.n_seg), B,
              0 if topn is None else min(int(topn), 0x7fffffff), 1 if list_mean else 0, 1 if reduce else 0,
              *[P(out.get(k)) for k in ('loss', 'n_valid', 'dbase', 'row_rank', 'group_loss', 'position', 'row_lse', 'list_loss', 'list_valid')],
              P(ws), ws.numel(), _lib.stream())
    return seg, B, out


class _ListMLE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, group_ids, labels, weights, mask, topn, list_mean, do_reduce):
        seg, B, out = _run(group_ids, labels, logits, weights, mask, topn, list_mean, do_reduce, True, False)
        n_valid = out['n_valid'].to(torch.float32)
        ctx.shape, ctx.do_reduce = logits.shape, do_reduce
        ctx.mark_non_differentiable(n_valid)
        if do_reduce:
            ctx.save_for_backward(out['dbase'][:B])
            return out['loss'], n_valid
        gv = int(out['n_valid'].item())
        if gv < 0:
            raise RuntimeError('rec_now_amd: the cooperative grouping kernel timed out at a grid barrier (workgroups not co-resident)')
        if weights is not None and weights.numel() != gv:
            raise ValueError('weights must have one entry per valid list: %d lists, %d weights' % (gv, weights.numel()))
        ctx.save_for_backward(out['dbase'][:B], out['row_rank'][:B])
        return out['group_loss'][:gv].clone(), n_valid

    @staticmethod
    def backward(ctx, g, _gn):
        if ctx.do_reduce:
            (dbase,) = ctx.saved_tensors           # already divided by the number of valid lists
            d = dbase * g
        else:
            dbase, row_rank = ctx.saved_tensors
            idx = torch.clamp(row_rank, min=0).long()
            gg = g[idx] if g.numel() > 0 else torch.zeros_like(dbase)
            d = torch.where(row_rank >= 0, dbase * gg, torch.zeros_like(dbase))
        return d.reshape(ctx.shape), None, None, None, None, None, None, None


def listmle_loss_from_batch(group_ids, labels, logits, weights=None, mask=None, topn=None, list_mean=False, do_reduce=True,
                            return_num_list=False):
    """The ListMLE loss of the lists of the batch (module docstring), differentiable in `logits`.  `weights`: (n_valid,) in first-occurrence
    order of the valid lists.  do_reduce=True: the mean over the valid lists as a 0-dim tensor, no host synchronisation; do_reduce=False: the
    (n_valid,) per-list losses.  Returns loss [, number of valid lists as a float tensor]."""
    _check(group_ids, labels, logits, weights, mask, topn)
    loss, n_valid = _ListMLE.apply(logits, group_ids, labels, weights, mask, topn, bool(list_mean), bool(do_reduce))
    return (loss, n_valid) if return_num_list else loss


def listmle_terms(group_ids, labels, logits, mask=None, topn=None):
    """What the loss is made of, ListMLETerms(position, lse, list_loss, valid):
      position (B,) int32     0-based place of the row in its list's permutation, -1 if it does not take part
      lse (B,) float64        lse_p of the row's place, NaN where position is -1
      list_loss (G,) float64  per list in first-occurrence order: the loss, unweighted and before 1/K
      valid (G,) bool
    Host-synchronises once (the number of lists).  No gradient."""
    seg, B, out = _run(group_ids, labels, logits, None, mask, topn, False, False, False, True)
    G = seg.num_segments() if B > 0 else 0
    first_row = seg.order[seg.seg_first[:G].long()]            # the smallest row of every segment: the caller's order is ascending inside one
    by_first = torch.argsort(first_row)
    return ListMLETerms(out['position'][:B], out['row_lse'][:B], out['list_loss'][:G][by_first], out['list_valid'][:G][by_first] != 0)
