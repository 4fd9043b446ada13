"""In-batch ApproxNDCG (Qin, Liu and Li 2010; `approx_ndcg_loss` of TF-Ranking): a differentiable NDCG loss.  It optimises NDCG itself, through
soft positions, where the pairwise losses optimise a surrogate.  An addition; the reference has no such loss.

Lists and rows.  A list is one segment of `build_segments(groups)`.  These are the lists of `in_batch_ndcg`: the pairwise equality rule, and
a list of group tensors means agreement in every one.  A row takes part when `mask` is true there, or when there is no mask.  Rows that do not
take part influence nothing and get gradient exactly 0.

Temperature.  `temperature` tau is a finite float greater than 0.  The default is 0.1.

Soft position of a taking-part row.  `R_i = sum_{j in the list, taking part, j != i} sigma((s_j - s_i) / tau)`.  It is 0-based, so it matches
`D(r) = 1 / log2(2 + r)` of `ndcg.py`.  For distinct scores, `R_i` tends to the hard position `r_i` as tau -> 0.

Gain.  `G(y)` is `2**y - 1` ('exp2') or `y` ('linear'), as in `ndcg.py`.

Ideal DCG.  `IDCG = sum G(y_i) D(q_i)`, with `q_i` the label position of `ndcg.py`.  Ties go to the smaller original row index.  There is no
`topn`.

Valid list.  A list is valid when `IDCG > 0`.  A NaN label of a taking-part row makes that comparison false, so the list is invalid, as it is
for `in_batch_ndcg`.

Loss of a valid list.  `l = -ADCG / IDCG`, with `ADCG = sum_i G(y_i) / log2(2 + R_i)`.  So `l` is in [-1, 0] for non-negative gains.  The batch
loss is the mean of `l` over the valid lists.  It is 0 when there is none.

Gradient.  `c_i = G(y_i) ln 2 / ((2 + R_i) ln^2(2 + R_i))` is `-G f'(R_i)` for `f(R) = 1 / log2(2 + R)`.  `sigma'_kj = sigma(x)(1 - sigma(x))`
with `x = (s_j - s_k) / tau`; it is symmetric in k and j.  Then `dl/ds_k = (1 / (tau IDCG)) sum_{j != k, taking part} sigma'_kj (c_j - c_k)`.
The gradient of a list sums to zero.  Rows of an invalid list get exactly 0.

NaN scores.  A NaN score of a taking-part row makes its own list's loss NaN (its `R` is NaN, also in a list of one).  The batch mean then
becomes NaN too.  That list's taking-part rows get NaN gradients.  Every other list's gradient bits stay as they were.  A row that does not
take part may hold any score and any label, NaN included, without changing one bit of any output.

Where the grouping reports a grid-barrier time-out, the loss and the gradient are NaN and the number of lists is -1.

Two pair walks on the skeletons of the pairwise losses, float32 sigmoids with fp64 accumulators, fp64 list sums in fixed order, no pair list,
no atomics, no host synchronisation, bitwise reproducible (csrc/pairwise_approx.hip, recnow_approx_ndcg_fwdbwd)."""
import collections
import math
import numbers

import torch

from .. import _lib
from ._segments import _inputs
from .ndcg import _GAIN_CODE

ApproxNDCGTerms = collections.namedtuple('ApproxNDCGTerms', ['approx_rank', 'list_adcg', 'list_idcg', 'loss_sum', 'n_lists'])


def _numel(t):
    if isinstance(t, (list, tuple)) and len(t) > 0 and all(isinstance(g, torch.Tensor) for g in t):
        return t[0].numel()
    return t.numel() if isinstance(t, torch.Tensor) else len(t)


def _check(outputs, labels, groups, mask, gain, temperature, segments):
    """The argument errors that need no device."""
    if not isinstance(gain, str) or gain not in _GAIN_CODE:
        raise ValueError("gain must be 'exp2' or 'linear', got %r" % (gain,))
    if isinstance(temperature, bool) or not isinstance(temperature, numbers.Real) or not math.isfinite(temperature) or not temperature > 0:
        raise ValueError('temperature must be a finite number greater than 0, got %r' % (temperature,))
    if not 1e-30 <= float(temperature) <= 1e30:          # the kernels take it, and 1 / it, as float32
        raise ValueError('temperature must lie in [1e-30, 1e30], got %r' % (temperature,))
    B = segments.B if segments is not None else _numel(groups)
    for t, what in ((outputs, 'outputs'), (labels, 'labels'), (mask, 'mask')):
        if t is not None and t.numel() != B:
            raise ValueError('outputs, labels, groups and mask must have the same number of elements: %d rows, %d %s' % (B, t.numel(), what))
    if segments is None and isinstance(groups, (list, tuple)) and any(isinstance(g, torch.Tensor) and g.numel() != B for g in groups):
        raise ValueError('all group tensors must have the same number of elements')
    return B


def _run(outputs, labels, groups, mask, gain, temperature, segments, want_grad, want_terms):
    _check(outputs, labels, groups, mask, gain, temperature, segments)
    seg, scores, labs, m = _inputs(outputs, labels, groups, mask, segments)
    B, dev = seg.B, seg.device
    n = max(B, 1)
    out = {'loss': torch.empty((), dtype=torch.float32, device=dev), 'loss_sum': torch.empty((), dtype=torch.float64, device=dev),
           'n_lists': torch.empty((), dtype=torch.int64, device=dev)}
    if want_grad:
        out['dscores'] = torch.empty(n, dtype=torch.float32, device=dev)
    if want_terms:
        out['approx_rank'], out['list_adcg'], out['list_idcg'] = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
    P = _lib.ptr
    ws = _lib.workspace(_lib.load().recnow_approx_ndcg_workspace_bytes(B), dev)
    _lib.call('recnow_approx_ndcg_fwdbwd', P(scores), P(labs), P(m), P(seg.order), P(seg.seg_id), P(seg.seg_first), P(seg.n_seg), B,
              _GAIN_CODE[gain], float(temperature),
              *[P(out.get(k)) for k in ('loss', 'loss_sum', 'n_lists', 'dscores', 'approx_rank', 'list_adcg', 'list_idcg')],
              P(ws), ws.numel(), _lib.stream())
    return seg, B, out


class _ApproxNDCG(torch.autograd.Function):
    @staticmethod
    def forward(ctx, outputs, labels, groups, mask, gain, temperature, segments):
        seg, B, out = _run(outputs, labels, groups, mask, gain, temperature, segments, True, False)
        n_lists = out['n_lists'].to(torch.float32)
        ctx.shape, ctx.dtype = outputs.shape, outputs.dtype
        ctx.save_for_backward(out['dscores'][:B])          # already divided by the number of valid lists
        ctx.mark_non_differentiable(n_lists)
        return out['loss'], n_lists

    @staticmethod
    def backward(ctx, g, _gn):
        (d,) = ctx.saved_tensors
        return (d * g).reshape(ctx.shape).to(ctx.dtype), None, None, None, None, None, None


def approx_ndcg_loss(outputs, labels, groups, mask=None, gain='exp2', temperature=0.1, segments=None, return_num_list=False):
    """The ApproxNDCG loss of the lists of the batch (module docstring) as a 0-dim float32 tensor, differentiable in `outputs`: the gradient is
    computed in the forward call and scaled by the upstream gradient in backward.  No host synchronisation; the call can be captured in a HIP
    graph.  segments: a precomputed `build_segments(groups)` (`groups` is then not looked at).  Returns loss [, number of valid lists as a
    float tensor]."""
    _check(outputs, labels, groups, mask, gain, temperature, segments)
    loss, n_lists = _ApproxNDCG.apply(outputs, labels, groups, mask, gain, temperature, segments)
    return (loss, n_lists) if return_num_list else loss


def approx_ndcg_terms(outputs, labels, groups, mask=None, gain='exp2', temperature=0.1, segments=None):
    """What the loss is made of, ApproxNDCGTerms(approx_rank, list_adcg, list_idcg, loss_sum, n_lists):
      approx_rank (B,) float64     R_i per original row, NaN for a row that does not take part
      list_adcg, list_idcg (B,) float64   per SEGMENT in sorted numbering: the first n_seg entries are written
      loss_sum 0-dim float64       the sum of l over the valid lists (with n_lists: what a caller all-reduces for a cross-rank mean)
      n_lists 0-dim int64          the number of valid lists
    No host synchronisation, no gradient."""
    seg, B, out = _run(outputs, labels, groups, mask, gain, temperature, segments, False, True)
    return ApproxNDCGTerms(out['approx_rank'][:B], out['list_adcg'][:B], out['list_idcg'][:B], out['loss_sum'], out['n_lists'])
