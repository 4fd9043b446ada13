"""In-batch pairwise ranking loss -- drop-in for rec_now/rec_block/pairwise_loss_from_batch.py.

Same public names, argument order, defaults and return structure as the reference
(/root/reference/rec_now/rec_block/pairwise_loss_from_batch.py), with torch.Tensor in place of tf.Tensor.  Underneath,
the reference's dense O(B^2) masks are replaced by sort-by-group + segmented pair enumeration in hand-written HIP
kernels (csrc/scan_sort.hip, csrc/pairwise.hip); pair order, counts and weights are identical to the reference's.

Two execution paths:
  * fused   -- `pairloss_func` is `bpr_loss_func` (or a functools.partial of it that binds only `factor` / `reduce_mean`), or one of
               `hinge_loss_func` / `squared_hinge_loss_func` / `margin_bpr_loss_func` (or a functools.partial binding only `margin` /
               `factor` / `reduce_mean`), and `label_pair_to_weight_func` is None or a `LabelPairWeightTable`: loss and
               d(loss)/d(outputs) come out of one kernel, pairs are never materialised; `lambda_weight=NDCGLambdaWeight(...)` (the
               LambdaRank pair weight, rec_block/ndcg.py) stays on this route as well (csrc/pairwise_lambda.hip);
  * general -- any other callable: pairs are materialised (bit-exact reference order), labels/outputs are gathered to
               (P,) vectors and the user's callables run on those.  Exact for element-wise callables (what the
               reference's own test uses, tests/rec_block/test_pairwise_loss_from_batch.py:51-53); callables that
               inspect the (B,B) *shape* are not supported.
"""
import collections
import functools
import math
import numbers
import os

import torch

from .. import _lib
from ._segments import _FLAG_MEMBERS_PACKED, _KEY_F64, _KEY_I64, Segments, _as_key_tensor, _flat_f32, _flat_mask, _inputs, build_segments
from .ndcg import NDCGLambdaWeight, lambda_workspace, ndcg_rank_terms, rank_terms_packed

SMALL_POSIVITE_FLOAT = 1.0E-10   # reference :13 (spelling kept)

_ONE_CALL = os.environ.get('RECNOW_PAIR_ONE_CALL', '1') != '0'      # A/B switch: '0' keeps the piecewise host route
_FLAG_LABEL_GT, _FLAG_WRONG_ORDER = 1, 2


def _generate_pair_mask(sample_group_idx_var, only_upper_band=False):
    """(B,B) bool mask of same-group, off-diagonal pairs (reference :16-40)."""
    return generate_pair_mask(sample_group_idx_var, only_upper_band)


def generate_pair_mask(group_tensor_or_list, only_upper_band=False):
    """Dense (B,B) bool mask, True where rows i != j share a group in every tensor of the list (reference :43-74).
    `only_upper_band=True` keeps only the first super-diagonal, exactly like tf.linalg.band_part(m, 0, 1) (:38-39).
    Provided for API parity; `pairwise_loss` itself never builds this matrix."""
    groups = list(group_tensor_or_list) if isinstance(group_tensor_or_list, (list, tuple)) else [group_tensor_or_list]
    seg = build_segments(groups)
    B = seg.B
    out = torch.zeros((B, B), dtype=torch.uint8, device=seg.device)
    _lib.call('recnow_pair_mask_dense', _lib.ptr(seg.order), _lib.ptr(seg.seg_id), _lib.ptr(seg.seg_first), B,
              1 if only_upper_band else 0, _lib.ptr(out), _lib.stream())
    return out.to(torch.bool)


def vec_to_matrix_pair(vec):
    """(B,1)/(1,B) vector -> (M, M^T) with M[i,j] = v_i (reference :77-93).  Returned as broadcast views."""
    vec = vec.reshape(-1, 1)
    mat = vec.expand(vec.shape[0], vec.shape[0])
    return mat, mat.t()


class _BprVec(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, neg, weights, factor, reduce_mean):
        shape = pos.shape
        p = _lib.f32c(pos, 'outputs_pos').reshape(-1)
        n = _lib.f32c(neg, 'outputs_neg').reshape(-1)
        if p.numel() != n.numel():
            raise ValueError('outputs_pos and outputs_neg must have the same number of elements')
        w = None
        if weights is not None:
            w = _lib.f32c(weights, 'weights').reshape(-1)
            if w.numel() != p.numel():
                w = w.expand_as(p).contiguous()
        P = p.numel()
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        dpos = torch.empty(max(P, 1), dtype=torch.float32, device=p.device)
        ws = _lib.workspace(1024 * 8 + 256, p.device)
        _lib.call('recnow_bpr_loss_fwdbwd', _lib.ptr(p), _lib.ptr(n), _lib.ptr(w), P, float(factor),
                  1 if reduce_mean else 0, _lib.ptr(loss), _lib.ptr(dpos), _lib.ptr(ws), ws.numel(), _lib.stream())
        ctx.save_for_backward(dpos[:P])
        ctx.shape = shape
        ctx.neg_shape = neg.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        (dpos,) = ctx.saved_tensors
        gp = dpos * g
        return gp.reshape(ctx.shape), (-gp).reshape(ctx.neg_shape), None, None, None


def bpr_loss_func(outputs_pos, outputs_neg, weights=None, factor=1.0, reduce_mean=True):
    """BPR / logistic pair loss on explicit vectors (reference :96-127):
    sum(w * softplus(-factor*(pos-neg))) / (P + 1e-10)   (raw sum when reduce_mean=False).  weights are constants."""
    return _BprVec.apply(outputs_pos, outputs_neg, weights, factor, reduce_mean)


_KIND_HINGE, _KIND_SQUARED_HINGE, _KIND_MARGIN_LOGISTIC = 1, 2, 3      # RECNOW_PAIR_KIND_* of include/recnow.h


def _finite_number(value, what):
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not math.isfinite(value):
        raise ValueError('%s must be a finite Python number, got %r' % (what, value))
    return float(value)


def _kind_loss_vec(kind, outputs_pos, outputs_neg, weights, margin, factor, reduce_mean):
    """sum(weights * f(margin - factor * (pos - neg))) [/ (P + 1e-10)] in plain torch ops on the tensors' own device: what the general
    route runs when one of the three functions below reaches it inside a lambda.  Not a hot path (`pairwise_loss` fuses the functions
    themselves and never comes here)."""
    margin, factor = _finite_number(margin, 'margin'), _finite_number(factor, 'factor')
    u = margin - factor * (outputs_pos - outputs_neg)
    if kind == _KIND_HINGE:
        losses = torch.relu(u)                                     # subgradient 0 at u == 0
    elif kind == _KIND_SQUARED_HINGE:
        losses = torch.relu(u) ** 2
    else:
        losses = torch.nn.functional.softplus(u)
    n = losses.numel()
    if weights is not None:
        losses = losses * torch.as_tensor(weights).detach()        # weights are constants
    loss = losses.sum()
    if reduce_mean:
        loss = loss / (float(n) + SMALL_POSIVITE_FLOAT)
    return loss


def hinge_loss_func(outputs_pos, outputs_neg, weights=None, margin=1.0, factor=1.0, reduce_mean=True):
    """Margin ranking (hinge) pair loss on explicit vectors, with the calling convention of `bpr_loss_func`:
    sum(w * max(margin - factor*(pos-neg), 0)) / (P + 1e-10)   (raw sum when reduce_mean=False); P counts every pair, also those whose
    term is 0.  weights are constants; the subgradient at the kink is 0.  As `pairloss_func` of `pairwise_loss` it stays on the fused route."""
    return _kind_loss_vec(_KIND_HINGE, outputs_pos, outputs_neg, weights, margin, factor, reduce_mean)


def squared_hinge_loss_func(outputs_pos, outputs_neg, weights=None, margin=1.0, factor=1.0, reduce_mean=True):
    """Squared hinge pair loss: sum(w * max(margin - factor*(pos-neg), 0)**2) / (P + 1e-10); otherwise as `hinge_loss_func`."""
    return _kind_loss_vec(_KIND_SQUARED_HINGE, outputs_pos, outputs_neg, weights, margin, factor, reduce_mean)


def margin_bpr_loss_func(outputs_pos, outputs_neg, weights=None, margin=1.0, factor=1.0, reduce_mean=True):
    """BPR / logistic pair loss with a margin: sum(w * softplus(margin - factor*(pos-neg))) / (P + 1e-10); otherwise as `hinge_loss_func`."""
    return _kind_loss_vec(_KIND_MARGIN_LOGISTIC, outputs_pos, outputs_neg, weights, margin, factor, reduce_mean)


_KIND_NAME_OF_FUNC = {hinge_loss_func: 'hinge', squared_hinge_loss_func: 'squared_hinge', margin_bpr_loss_func: 'margin_bpr'}
_KIND_OF_NAME = {'hinge': _KIND_HINGE, 'squared_hinge': _KIND_SQUARED_HINGE, 'margin_bpr': _KIND_MARGIN_LOGISTIC}


def occurance_power_weight(group_id, power=0.0):
    """weights[i] = (number of elements sharing group_id[i]) ** power (reference :130-151)."""
    seg = build_segments(group_id)
    w = torch.empty(max(seg.B, 1), dtype=torch.float32, device=seg.device)
    _lib.call('recnow_occurance_power_weight', _lib.ptr(seg.order), _lib.ptr(seg.seg_id), _lib.ptr(seg.seg_first), seg.B,
              float(power), _lib.ptr(w), _lib.stream())
    return w[:seg.B]


def _pair_flags(table, wrong, label_cond=True):
    """The predicate flags of a pair rule: a LabelPairWeightTable carries its own label rule, the default rule is label_i > label_j."""
    return (_FLAG_LABEL_GT if table is None and label_cond else 0) | (_FLAG_WRONG_ORDER if wrong else 0)


def _table_args(table, device):
    """(label_values, n_values, weights) of a LabelPairWeightTable as a library entry takes them; (NULL, 0, NULL) without one."""
    if table is None:
        return None, 0, None
    vals, w = table.on_device(device)
    return _lib.ptr(vals), table.n_values, _lib.ptr(w)


def _pair_workspace(B, device):
    return _lib.workspace(_lib.load().recnow_pairwise_workspace_bytes(B), device)


def _counters(B, device):
    """(cnt_super, n_pair): the pair counts per main group and of the batch."""
    return torch.empty(max(B, 1), dtype=torch.int64, device=device), torch.empty(1, dtype=torch.int64, device=device)


def _count(seg, scores, labs, m, table, wrong, extra_flags, ws, label_cond=True, counters=None):
    """The counting entry of the pair rule on `ws` -- recnow_pair_table_count with a LabelPairWeightTable, else recnow_pair_count -- and the
    only call site of both.  extra_flags: _FLAG_MEMBERS_PACKED after recnow_group_pack_small on the same `ws`, which has then cleared the
    `counters` (cnt_super, n_pair) as well; without them they are allocated here.  Returns (flags, cnt_row, cnt_super, n_pair): the predicate
    flags, and the pair counts per row / main group / batch; the members stay packed in `ws` for the loss entry that follows."""
    B, dev = seg.B, seg.device
    cnt_row = torch.empty(max(B, 1), dtype=torch.int32, device=dev)
    cnt_super, n_pair = counters if counters is not None else _counters(B, dev)
    flags = _pair_flags(table, wrong, label_cond)
    P = _lib.ptr
    rows = (P(scores), P(labs), P(m), P(seg.order), P(seg.seg_id), P(seg.seg_first), P(seg.super_id), B, flags | extra_flags)
    outs = (P(cnt_row), P(cnt_super), P(n_pair), P(ws), ws.numel(), _lib.stream())
    if table is None:
        _lib.call('recnow_pair_count', *rows, *outs)
    else:
        _lib.call('recnow_pair_table_count', *rows, *_table_args(table, dev), *outs)
    return flags, cnt_row, cnt_super, n_pair


def pair_indices(outputs, labels, groups, only_use_wrong_order_pair=False, mask=None, use_label_cond=True):
    """(pos_idx, neg_idx) int32 tensors of the surviving pairs in the reference's order: ascending positive row i,
    then ascending negative row j (= tf.boolean_mask over the row-major flattened (B,B) mask, reference :217,272-273).
    Host-synchronises once to size the output."""
    seg, scores, labs, m = _inputs(outputs, labels, groups, mask, None)
    B = seg.B
    ws = _pair_workspace(B, seg.device)
    flags, cnt_row, _, n_pair = _count(seg, scores, labs, m, None, only_use_wrong_order_pair, 0, ws, label_cond=use_label_cond)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=seg.device)
    _lib.call('recnow_pair_offsets', _lib.ptr(cnt_row), B, _lib.ptr(offsets), _lib.ptr(ws), ws.numel(), _lib.stream())
    P = int(n_pair.item())
    pos = torch.empty(max(P, 1), dtype=torch.int32, device=seg.device)
    neg = torch.empty(max(P, 1), dtype=torch.int32, device=seg.device)
    _lib.call('recnow_pair_emit', _lib.ptr(scores), _lib.ptr(labs), _lib.ptr(m), _lib.ptr(seg.order), _lib.ptr(seg.seg_id),
              _lib.ptr(seg.seg_first), B, flags, _lib.ptr(offsets), _lib.ptr(pos), _lib.ptr(neg), P, _lib.ptr(ws),
              ws.numel(), _lib.stream())
    return pos[:P], neg[:P]


def _n_pair_out(ctx, n_pair):
    """The pair count as the float32 0-dim tensor the reference returns -- only when the caller asked for it (one conversion kernel
    and its host time less on the default `pairwise_loss(...)` path)."""
    if not ctx.want_np:
        return None
    n_pair_f = n_pair.to(torch.float32).reshape(())
    ctx.mark_non_differentiable(n_pair_f)
    return n_pair_f


class LabelPairWeightTable(object):
    """An element-wise `label_pair_to_weight_func` over labels that take at most 16 distinct values, as a K x K table: `weights[a, b]`
    is the weight of a pair whose positive row has label `label_values[a]` and whose negative row has label `label_values[b]`.  Passed as
    `pairwise_loss(..., label_pair_to_weight_func=table)` it keeps the call on the fused route (csrc/pairwise_table.hip); it is also an
    ordinary weight callable (lookup with torch ops, NaN for a label outside the values), so every other route takes it as well.

    label_values: 1..16 distinct finite values (list, numpy or tensor), stored and compared as float32 (-0.0 equals 0.0).
    The table comes from `weights` ((K, K), kept as given), or from ONE call of `label_pair_to_weight_func(M, M^T, **kwargs)` on the
    (K, K) broadcast matrices of the values -- as the reference calls it on its (B, B) label matrices (:187-193) --, or, with neither,
    from the default rule: 1.0 where values[a] > values[b], else 0.  As in the reference (:193) a pair survives where its weight is > 0:
    zero, negative and NaN entries drop the pair, +inf keeps it."""

    MAX_VALUES = 16

    def __init__(self, label_values, label_pair_to_weight_func=None, weights=None, **kwargs):
        vals = torch.as_tensor(label_values).detach().to('cpu', torch.float32).reshape(-1).clone()
        K = vals.numel()
        if K == 0:
            raise ValueError('label_values must hold at least one value')
        if K > self.MAX_VALUES:
            raise ValueError('label_values holds %d values, at most %d are supported' % (K, self.MAX_VALUES))
        if not bool(torch.isfinite(vals).all()):
            raise ValueError('label_values must be finite (as float32)')
        if int((vals.reshape(-1, 1) == vals.reshape(1, -1)).sum()) != K:
            raise ValueError('label_values must be distinct (compared as float32; -0.0 equals 0.0)')
        if weights is not None and label_pair_to_weight_func is not None:
            raise ValueError('pass either weights or label_pair_to_weight_func, not both')
        if kwargs and label_pair_to_weight_func is None:
            raise ValueError('keyword arguments %s are for label_pair_to_weight_func, which was not given' % sorted(kwargs))
        if weights is not None:
            w = torch.as_tensor(weights).detach().to('cpu', torch.float32).clone()
        elif label_pair_to_weight_func is not None:
            a, b = vec_to_matrix_pair(vals)
            w = torch.as_tensor(label_pair_to_weight_func(a.clone(), b.clone(), **kwargs)).detach().to('cpu', torch.float32).clone()
        else:
            a, b = vec_to_matrix_pair(vals)
            w = (a > b).to(torch.float32)
        if tuple(w.shape) != (K, K):
            raise ValueError('the weight table must have shape (%d, %d), got %s' % (K, K, tuple(w.shape)))
        self.label_values = vals
        self.weights = w.contiguous()
        self.n_values = K
        self._per_device = {}

    def on_device(self, device):
        """(label_values, weights) as float32 tensors on `device`, uploaded once per device."""
        device = torch.device(device)
        if device.type == 'cpu':
            return self.label_values, self.weights
        hit = self._per_device.get(device)
        if hit is None:
            hit = (self.label_values.to(device), self.weights.to(device).contiguous())
            self._per_device[device] = hit
        return hit

    def __call__(self, label_pos, label_neg, **ignored):
        lp, ln = torch.as_tensor(label_pos), torch.as_tensor(label_neg)
        vals, w = self.on_device(lp.device)
        lp, ln = torch.broadcast_tensors(lp.to(torch.float32), ln.to(device=lp.device, dtype=torch.float32))
        hit_p, hit_n = lp.unsqueeze(-1) == vals, ln.unsqueeze(-1) == vals
        out = w[hit_p.to(torch.uint8).argmax(-1), hit_n.to(torch.uint8).argmax(-1)]
        return torch.where(hit_p.any(-1) & hit_n.any(-1), out, torch.full_like(out, float('nan')))


# What a fused call computes, apart from its rows and their grouping.  table: a LabelPairWeightTable or None (label_i > label_j); wrong:
# only_use_wrong_order_pair; kind: a _KIND_* code, or None for the BPR term; lam: an NDCGLambdaWeight or None (then kind is never None: BPR is
# the margin-logistic kind at margin 0 there); power: click_occurance_power.
_PairPlan = collections.namedtuple('_PairPlan', ['table', 'wrong', 'kind', 'margin', 'factor', 'power', 'reduce_mean', 'lam'])


def _pack_small(gkey, gdt, scores, labs, m, counters, ws):
    """Keys, grouping and member packing of B <= 8192 rows of one float32 / int32 group tensor in ONE launch (recnow_group_pack_small); it
    clears `counters` as well, so what follows on `ws` runs with _FLAG_MEMBERS_PACKED.  Returns the Segments."""
    seg = Segments()
    B, dev = gkey.numel(), gkey.device
    seg.B, seg.device = B, dev
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)      # noqa: E731
    seg.order, seg.seg_id, seg.seg_first, seg.super_id, seg.n_seg = i32(max(B, 1)), i32(max(B, 1)), i32(B + 1), i32(max(B, 1)), i32(2)
    _lib.call('recnow_group_pack_small', _lib.ptr(gkey), gdt, _lib.ptr(labs), _lib.ptr(scores), _lib.ptr(m), B, _lib.ptr(seg.order),
              _lib.ptr(seg.seg_id), _lib.ptr(seg.seg_first), _lib.ptr(seg.super_id), _lib.ptr(seg.n_seg), _lib.ptr(counters[0]),
              _lib.ptr(counters[1]), _lib.ptr(ws), ws.numel(), _lib.stream())
    return seg


class _PairFused(torch.autograd.Function):
    """Every fused route that walks segments.  grouping: a Segments, or the (key tensor, dtype code) of `_small_route`, grouped here by
    `_pack_small`.  plan: a _PairPlan.  Then, all on ONE workspace, with no host synchronisation and nothing sized by the number of pairs:
      * plain BPR without occurrence weights (power == 0): counts and terms from ONE walk per row (recnow_pair_bpr_onepass); the gradient stays
        unnormalised until backward multiplies the incoming gradient in (recnow_pair_scale_grad);
      * otherwise `_count`, the rank pre-pass (recnow_pair_lambda_terms) when the plan has a lambda weight, and the one loss entry of the
        plan: recnow_pair_lambda_fwdbwd, recnow_pair_kind_fwdbwd, recnow_pair_table_bpr_fwdbwd or recnow_pair_bpr_fwdbwd, on the packed
        members the count left behind.  The lambda route's workspace is the larger one of its walk, from the count on."""

    @staticmethod
    def forward(ctx, outputs, labels, mask, grouping, plan, want_np=True):
        small = not isinstance(grouping, Segments)
        B, dev = (grouping[0].numel(), grouping[0].device) if small else (grouping.B, grouping.device)
        ctx.want_np = bool(want_np)
        ctx.shape = outputs.shape
        scores = _flat_f32(outputs, B, 'outputs')
        labs = _flat_f32(labels, B, 'labels')
        m = _flat_mask(mask, B)
        table, lam = plan.table, plan.lam
        ws = lambda_workspace(B, dev) if lam is not None else _pair_workspace(B, dev)
        ctx.onepass = plan.kind is None and table is None and float(plan.power) == 0.0
        counters, packed = None, 0
        if small:
            counters, packed = _counters(B, dev), _FLAG_MEMBERS_PACKED
            seg = _pack_small(grouping[0], grouping[1], scores, labs, m, counters, ws)
        else:
            seg = grouping
        P, st = _lib.ptr, _lib.stream()
        rows = (P(scores), P(labs), P(m), P(seg.order))
        loss = torch.empty((), dtype=torch.float32, device=dev)
        dscores = torch.empty(max(B, 1), dtype=torch.float32, device=dev)
        rm = 1 if plan.reduce_mean else 0
        if ctx.onepass:
            n_pair = counters[1] if small else torch.empty(1, dtype=torch.int64, device=dev)
            _lib.call('recnow_pair_bpr_onepass', *rows, P(seg.seg_id), P(seg.seg_first), B, _pair_flags(None, plan.wrong) | packed,
                      float(plan.factor), rm, P(loss), P(dscores), P(n_pair), P(ws), ws.numel(), st)
            ctx.save_for_backward(dscores[:B], n_pair)
            ctx.reduce_mean = bool(plan.reduce_mean)
            return loss, _n_pair_out(ctx, n_pair)
        flags, _, cnt_super, n_pair = _count(seg, scores, labs, m, table, plan.wrong, packed, ws, counters=counters)
        segs = (P(seg.seg_id), P(seg.seg_first), P(seg.super_id), P(cnt_super), P(n_pair), B, flags | _FLAG_MEMBERS_PACKED)
        outs = (float(plan.factor), float(plan.power), rm, P(loss), P(dscores), P(ws), ws.numel(), st)
        targs = _table_args(table, dev)
        if lam is not None:
            rank_terms_packed(seg, ws, lam.gain, lam.topn)
            _lib.call('recnow_pair_lambda_fwdbwd', *segs, int(plan.kind), float(plan.margin), targs[1], targs[2], *outs)
        elif plan.kind is not None:
            _lib.call('recnow_pair_kind_fwdbwd', *rows, *segs, int(plan.kind), float(plan.margin), *targs, *outs)
        elif table is not None:         # its own entry, not the kind entry at margin 0
            _lib.call('recnow_pair_table_bpr_fwdbwd', *rows, *segs, *targs, *outs)
        else:
            _lib.call('recnow_pair_bpr_fwdbwd', *rows, *segs, *outs)
        ctx.save_for_backward(dscores[:B])
        return loss, _n_pair_out(ctx, n_pair)

    @staticmethod
    def backward(ctx, g, _g_np):
        saved = ctx.saved_tensors
        dscores = saved[0]
        if ctx.onepass:
            gd = g.detach().to(torch.float32).reshape(1).contiguous()
            grad = torch.empty_like(dscores)
            _lib.call('recnow_pair_scale_grad', _lib.ptr(dscores), _lib.ptr(gd), _lib.ptr(saved[1]) if ctx.reduce_mean else None, 1.0e-10,
                      dscores.numel(), _lib.ptr(grad), _lib.stream())
        else:
            grad = dscores * g
        return grad.reshape(ctx.shape), None, None, None, None, None


class _PairLossOneCall(torch.autograd.Function):
    """The default pairwise_loss (BPR, no occurrence weights, one group tensor) through ONE library call (recnow_pairwise_loss):
    grouping, loss and the gradient in a single ctypes call on two allocations (workspace; [d loss / d scores | loss | P]), the
    backward pass is one multiply.  Same kernels as the piecewise route; the host side of a B = 8192 loss drops from ~0.18 to ~0.1 ms."""

    @staticmethod
    def forward(ctx, outputs, labels, mask, gkey, gdt, flags, factor, reduce_mean, want_np):
        B = gkey.numel()
        scores = _flat_f32(outputs, B, 'outputs')
        labs = _flat_f32(labels, B, 'labels')
        m = _flat_mask(mask, B)
        dev = gkey.device
        lib = _lib.load()
        nws = lib.recnow_pairwise_loss_workspace_bytes(B, gdt)
        ws = torch.empty(nws + 8, dtype=torch.uint8, device=dev)          # + the int64 pair count at its (256-byte aligned) end
        out = torch.empty(B + 2, dtype=torch.float32, device=dev)         # [dscores (B) | loss | (float) P]
        n_pair_ptr = ws.data_ptr() + nws
        _lib.call('recnow_pairwise_loss', _lib.ptr(gkey), gdt, _lib.ptr(labs), _lib.ptr(scores), _lib.ptr(m), B, flags, float(factor),
                  1 if reduce_mean else 0, _lib._P(out.data_ptr() + 4 * B), _lib._P(n_pair_ptr), _lib._P(out.data_ptr() + 4 * B),
                  _lib.ptr(out), _lib.ptr(ws), nws, _lib.stream())
        ctx.save_for_backward(out)
        ctx.B = B
        ctx.shape = outputs.shape
        loss = out[B].reshape(())
        if not want_np:
            return loss, None
        n_pair_f = out[B + 1].reshape(())
        ctx.mark_non_differentiable(n_pair_f)
        return loss, n_pair_f

    @staticmethod
    def backward(ctx, g, _g_np):
        (out,) = ctx.saved_tensors
        return (out[:ctx.B] * g).reshape(ctx.shape), None, None, None, None, None, None, None, None


def _one_call_route(groups):
    """(key tensor, dtype code) when the one-call loss applies: ONE group tensor (any supported id dtype)."""
    if isinstance(groups, (list, tuple)):
        if len(groups) != 1:
            return None
        groups = groups[0]
    if not isinstance(groups, torch.Tensor) or not groups.is_cuda:
        return None
    try:
        return _as_key_tensor(groups)
    except TypeError:
        return None


def _small_route(groups):
    """(key tensor, dtype code) when the single-launch route applies: one group tensor of B <= 8192 float / int32-able ids."""
    one = _one_call_route(groups)
    if one is None or one[1] in (_KEY_F64, _KEY_I64) or not _lib.load().recnow_pairwise_small_supported(one[0].numel(), one[1]):
        return None
    return one


def group_rows(groups):
    """The score-independent half of the loss: canonical keys -> radix sort -> segments of `groups` (tensor or list of
    tensors, as `pairwise_loss` takes them).  The result can be handed to `pairwise_loss_fused(..., segments=...)`, so a
    training step can build it on a side stream while the model's forward pass is still producing the scores."""
    return build_segments(groups)


def pairwise_loss_fused(outputs, labels, groups, only_use_wrong_order_pair=False, click_occurance_power=0.0, mask=None,
                        factor=1.0, reduce_mean=True, segments=None, return_num_pair=True, label_pair_weights=None, *, kind=None, margin=0.0,
                        lambda_weight=None):
    """Fused pairwise loss; returns (loss, n_pair) as 0-dim tensors, no host sync.  `pairwise_loss` routes here
    whenever the defaults make it possible; exposed because it also accepts `factor` / `reduce_mean` and a precomputed
    `segments=group_rows(groups)` (then `groups` is not looked at again).  return_num_pair=False: the second value is None (the
    float32 conversion of the pair count is a kernel of its own).  label_pair_weights: a `LabelPairWeightTable` in place of the
    default rule "label_i > label_j, weight 1".
    kind (keyword only): None -- the BPR term softplus(-factor (s_i - s_j)), `margin` must stay 0 --, or 'hinge' / 'squared_hinge' /
    'margin_bpr': the term of `hinge_loss_func` / `squared_hinge_loss_func` / `margin_bpr_loss_func` on u = margin - factor (s_i - s_j)
    (csrc/pairwise_kind.hip).  margin (keyword only): a finite Python number.
    lambda_weight (keyword only): None, or an `NDCGLambdaWeight` -- every pair's weight is multiplied by the LambdaRank weight |delta NDCG| of
    the pair (rec_block/ndcg.py); the pair set, the pair count and the occurrence counts stay what they are without it.  The call then takes
    the segments route: count, rank pre-pass, lambda walk (csrc/pairwise_lambda.hip).
    Routes, in this precedence: lambda, kind, table -- each on `segments` or `build_segments(groups)` --, then for plain BPR the one-call
    entry (power 0, one group tensor, no `segments`), the small route (`_small_route`), the segments route."""
    if label_pair_weights is not None and not isinstance(label_pair_weights, LabelPairWeightTable):
        raise TypeError('label_pair_weights must be a LabelPairWeightTable, got %s' % type(label_pair_weights))
    if lambda_weight is not None and not isinstance(lambda_weight, NDCGLambdaWeight):
        raise TypeError('lambda_weight must be an NDCGLambdaWeight, got %s' % type(lambda_weight))
    if kind is None:
        if margin != 0.0:
            raise ValueError('margin needs a kind: the BPR term has none')
        kind_code = _KIND_MARGIN_LOGISTIC if lambda_weight is not None else None      # the lambda walk: softplus(-factor (s_i - s_j))
        margin = 0.0
    elif kind not in _KIND_OF_NAME:
        raise ValueError("kind must be None, 'hinge', 'squared_hinge' or 'margin_bpr', got %r" % (kind,))
    else:
        kind_code, margin = _KIND_OF_NAME[kind], _finite_number(margin, 'margin')
    if kind_code is not None:          # the kind and lambda entries demand a finite Python number; the BPR entries take float(factor)
        factor = _finite_number(factor, 'factor')
    wrong = bool(only_use_wrong_order_pair)
    plan = _PairPlan(label_pair_weights, wrong, kind_code, margin, factor, click_occurance_power, reduce_mean, lambda_weight)
    grouping = segments
    if grouping is None and kind_code is None and label_pair_weights is None:
        if float(click_occurance_power) == 0.0 and _ONE_CALL:
            one = _one_call_route(groups)
            if one is not None and one[0].numel() > 0:
                return _PairLossOneCall.apply(outputs, labels, mask, one[0], one[1], _pair_flags(None, wrong), factor, reduce_mean,
                                              return_num_pair)
        grouping = _small_route(groups)
    if grouping is None:
        grouping = build_segments(groups)
    return _PairFused.apply(outputs, labels, mask, grouping, plan, return_num_pair)


def _bpr_options(pairloss_func):
    """(factor, reduce_mean) when `pairloss_func` is `bpr_loss_func` itself or a functools.partial of it that binds nothing but the
    keywords `factor` / `reduce_mean` -- what the fused route can compute --, else None."""
    if pairloss_func is bpr_loss_func:
        return 1.0, True
    if (isinstance(pairloss_func, functools.partial) and pairloss_func.func is bpr_loss_func and not pairloss_func.args
            and set(pairloss_func.keywords) <= {'factor', 'reduce_mean'}):
        return pairloss_func.keywords.get('factor', 1.0), pairloss_func.keywords.get('reduce_mean', True)
    return None


def _kind_options(pairloss_func):
    """(kind name, margin, factor, reduce_mean) when `pairloss_func` is `hinge_loss_func`, `squared_hinge_loss_func` or `margin_bpr_loss_func`
    itself, or a functools.partial of one that binds no positional argument and nothing but the keywords `margin` / `factor` /
    `reduce_mean` -- what csrc/pairwise_kind.hip can compute --, else None.  A bound `margin` / `factor` that is no finite Python number
    raises ValueError here, as the function itself would on its first call."""
    func, kw = pairloss_func, {}
    if isinstance(pairloss_func, functools.partial):
        if pairloss_func.args or not set(pairloss_func.keywords) <= {'margin', 'factor', 'reduce_mean'}:
            return None
        func, kw = pairloss_func.func, pairloss_func.keywords
    try:
        name = _KIND_NAME_OF_FUNC.get(func)
    except TypeError:                       # an unhashable callable
        return None
    if name is None:
        return None
    return (name, _finite_number(kw.get('margin', 1.0), 'margin'), _finite_number(kw.get('factor', 1.0), 'factor'),
            bool(kw.get('reduce_mean', True)))


def _fused_options(pairloss_func):
    """The keyword arguments of `pairwise_loss_fused` that compute `pairloss_func` (`_bpr_options`, then `_kind_options`), else None."""
    bpr = _bpr_options(pairloss_func)
    if bpr is not None:
        return {'factor': bpr[0], 'reduce_mean': bpr[1]}
    kopt = _kind_options(pairloss_func)
    if kopt is not None:
        return {'kind': kopt[0], 'margin': kopt[1], 'factor': kopt[2], 'reduce_mean': kopt[3]}
    return None


def _merge_weights_by_mul(weights1, weights2):
    if weights1 is None:
        return weights2
    if weights2 is None:
        return weights1
    return weights1 * weights2


def pairwise_loss(outputs, labels, groups,
                  pairloss_func=bpr_loss_func,
                  only_use_wrong_order_pair=False,
                  return_num_pair=False,
                  click_occurance_power=0.0,
                  mask=None,
                  label_pair_to_weight_func=None,
                  lambda_weight=None,
                  **kwargs
                  ):
    """Pairwise loss over all in-batch pairs (i, j) of the same group with label_i > label_j (reference :228-279).

    Args (as the reference): outputs, labels: (B,)/(B,1) tensors; groups: tensor or list of tensors (AND of the
    conditions, groups[0] = main group for `click_occurance_power`); pairloss_func(outputs_pos, outputs_neg, weights);
    only_use_wrong_order_pair; return_num_pair; click_occurance_power; mask (bool, same shape as labels);
    label_pair_to_weight_func(label_pos, label_neg, **kwargs) -> weights, pairs with weight <= 0 are dropped; a
    `LabelPairWeightTable` keeps the call on the fused route (with bpr_loss_func, or a functools.partial of it binding factor / reduce_mean;
    with hinge_loss_func / squared_hinge_loss_func / margin_bpr_loss_func, or a functools.partial of one binding margin / factor / reduce_mean).
    lambda_weight: None, or an `NDCGLambdaWeight` (rec_block/ndcg.py): the LambdaRank weight |delta NDCG| of each pair, one more factor of
    the pair's weight beside the rule weight and the occurrence weight; it never changes which pairs exist.  Wherever the call is fused
    without it, it is fused with it; on the general route the weight is formed for the pair list from `ndcg_rank_terms`.
    Returns: loss, or (loss, n_pair as float32 tensor) when return_num_pair.
    """
    if lambda_weight is not None and not isinstance(lambda_weight, NDCGLambdaWeight):
        raise TypeError('lambda_weight must be an NDCGLambdaWeight, got %s' % type(lambda_weight))
    table = label_pair_to_weight_func if isinstance(label_pair_to_weight_func, LabelPairWeightTable) else None
    if table is not None and kwargs:
        raise ValueError('a LabelPairWeightTable took its keyword arguments when it was built; got %s' % sorted(kwargs))
    opts = _fused_options(pairloss_func) if (label_pair_to_weight_func is None or table is not None) else None
    if opts is not None:
        loss, n_pair = pairwise_loss_fused(outputs, labels, groups, only_use_wrong_order_pair, click_occurance_power, mask,
                                           return_num_pair=return_num_pair, label_pair_weights=table, lambda_weight=lambda_weight, **opts)
        return (loss, n_pair) if return_num_pair else loss

    # general path: materialise the pair list, then run the user's callables on (P,) vectors
    flat_out = _lib.require_gpu(outputs, 'outputs').reshape(-1)
    flat_lab = _lib.require_gpu(labels, 'labels').reshape(-1)
    pos, neg = pair_indices(outputs, labels, groups, only_use_wrong_order_pair, mask,
                            use_label_cond=label_pair_to_weight_func is None)
    weights = None
    if label_pair_to_weight_func is not None:
        w_all = label_pair_to_weight_func(flat_lab[pos.long()], flat_lab[neg.long()], **kwargs)   # reference :192
        keep = w_all > 0                                                                        # reference :193
        pos, neg, weights = pos[keep], neg[keep], w_all[keep]
    if click_occurance_power != 0.0:                                                            # reference :282-291
        group = groups[0] if isinstance(groups, (list, tuple)) else groups
        if pos.numel() > 0:
            occ = occurance_power_weight(group.reshape(-1)[pos.long()], power=click_occurance_power)
        else:
            occ = torch.empty(0, dtype=torch.float32, device=flat_out.device)
        weights = _merge_weights_by_mul(weights, occ)
    if lambda_weight is not None:
        terms = ndcg_rank_terms(outputs, labels, groups, mask=mask, gain=lambda_weight.gain, topn=lambda_weight.topn)
        pl, nl = pos.long(), neg.long()
        lam = (terms.gain[pl] - terms.gain[nl]).abs() * (terms.discount[pl] - terms.discount[nl]).abs() * terms.inv_idcg[pl]
        weights = _merge_weights_by_mul(weights, lam)
    if weights is not None:
        weights = weights.detach()                                                              # reference :269-270
    outputs_pos = flat_out[pos.long()]
    outputs_neg = flat_out[neg.long()]
    loss = pairloss_func(outputs_pos, outputs_neg, weights)                                     # reference :274
    if return_num_pair:
        return loss, torch.tensor(float(pos.numel()), dtype=torch.float32, device=flat_out.device)
    return loss
