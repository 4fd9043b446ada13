"""attention_by_dot_product and attention_by_dnn -- drop-ins for rec_now/rec_block/attention.py:12-38 and :41-82
(/root/reference/rec_now/rec_block/attention.py).  One fused HIP kernel per direction each: the dot product is HBM-bound (the
(B,L,D) user embeddings are read once forward, once backward with the scores recomputed); the DIN unit runs its Dense stack per
tile of positions on the exact-fp32 matrix cores without forming any (B,L,H) activation (csrc/attention_dnn.hip).
attention_by_softmax is an addition (the reference has no softmax attention): masked multi-head softmax target attention, one fused
kernel per direction that never forms the (B, H, L) scores (csrc/attention_softmax.hip)."""
import ctypes
import math

import torch

from .. import _lib
from ..layers._keras import Layer, activation_code


class _AttnDotFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, user_emb, doc_emb, filter_neg):
        u = _lib.f32c(user_emb, 'user_emb')
        d = _lib.f32c(doc_emb, 'doc_emb')
        if u.dim() != 3 or d.dim() != 2 or u.shape[0] != d.shape[0] or u.shape[2] != d.shape[1]:
            raise ValueError('user_emb must be (B, L, D) and doc_emb (B, D); got %s and %s' % (tuple(u.shape), tuple(d.shape)))
        B, L, D = u.shape
        if D > 256:
            raise NotImplementedError('attention_by_dot_product kernels cover embedding_dim <= 256 (the reference has no limit); got %d' % D)
        mat = torch.empty((B, D), dtype=torch.float32, device=u.device)
        ssum = torch.empty((B, 1), dtype=torch.float32, device=u.device)
        _lib.call('recnow_attention_dot_fwd', _lib.ptr(u), _lib.ptr(d), B, L, D, 1 if filter_neg else 0, _lib.ptr(mat),
                  _lib.ptr(ssum), _lib.stream())
        ctx.save_for_backward(u, d)
        ctx.filter_neg = bool(filter_neg)
        return mat, ssum

    @staticmethod
    def backward(ctx, dmat, dsum):
        u, d = ctx.saved_tensors
        B, L, D = u.shape
        dmat = _lib.f32c(dmat, 'grad') if dmat is not None else None
        dsum = _lib.f32c(dsum, 'grad').reshape(-1) if dsum is not None else None
        du = torch.empty_like(u)
        dd = torch.empty_like(d)
        _lib.call('recnow_attention_dot_bwd', _lib.ptr(u), _lib.ptr(d), _lib.ptr(dmat), _lib.ptr(dsum), B, L, D,
                  1 if ctx.filter_neg else 0, _lib.ptr(du), _lib.ptr(dd), _lib.stream())
        return du, dd, None


def attention_by_dot_product(user_emb, doc_emb, filter_neg=False):
    """Dot-product attention of L user-feature embeddings against one item embedding.

    Args:
        user_emb: (B, L, D);  doc_emb: (B, D);  filter_neg: clamp negative scores to 0 (:31-32).
    Returns:
        attn_mat (B, D) = sum_l user_emb[:, l] * score_l,  attn_score_sum (B, 1) = sum_l score_l.
    """
    return _AttnDotFunction.apply(user_emb, doc_emb, filter_neg)


_DIN_MAX_WIDTH = 256
_DIN_MAX_HIDDEN = 3


class _AttnDnnFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, user_emb, doc_emb, dims, act, *params):
        u = _lib.f32c(user_emb, 'user_emb')
        d = _lib.f32c(doc_emb, 'doc_emb')
        B, L, D = u.shape
        nl = len(dims)
        ks = [_lib.f32c(p, 'kernel') for p in params[:nl]]
        bs = [_lib.f32c(p, 'bias') for p in params[nl:]]
        dims_c = (ctypes.c_int * nl)(*dims)
        kp = (ctypes.c_void_p * nl)(*[k.data_ptr() for k in ks])
        bp = (ctypes.c_void_p * nl)(*[b.data_ptr() for b in bs])
        mat = torch.empty((B, D), dtype=torch.float32, device=u.device)
        ssum = torch.empty((B, 1), dtype=torch.float32, device=u.device)
        ws = _lib.workspace(_lib.load().recnow_attention_dnn_workspace_bytes(B, L, D, nl, dims_c, 0), u.device)
        _lib.call('recnow_attention_dnn_fwd', _lib.ptr(u), _lib.ptr(d), B, L, D, nl, dims_c, kp, bp, act, _lib.ptr(mat), _lib.ptr(ssum),
                  _lib.ptr(ws), ws.numel(), _lib.stream())
        ctx.save_for_backward(u, d, *ks, *bs)
        ctx.dims, ctx.act = tuple(dims), act
        return mat, ssum

    @staticmethod
    def backward(ctx, dmat, dsum):
        u, d, *params = ctx.saved_tensors
        dims, nl = ctx.dims, len(ctx.dims)
        ks, bs = params[:nl], params[nl:]
        B, L, D = u.shape
        dmat = _lib.f32c(dmat, 'grad') if dmat is not None else None
        dsum = _lib.f32c(dsum, 'grad').reshape(-1) if dsum is not None else None
        du, dd = torch.empty_like(u), torch.empty_like(d)
        dks = [torch.empty_like(k) for k in ks]
        dbs = [torch.empty_like(b) for b in bs]
        dims_c = (ctypes.c_int * nl)(*dims)
        ptrs = lambda ts: (ctypes.c_void_p * nl)(*[t.data_ptr() for t in ts])       # noqa: E731
        ws = _lib.workspace(_lib.load().recnow_attention_dnn_workspace_bytes(B, L, D, nl, dims_c, 1), u.device)
        _lib.call('recnow_attention_dnn_bwd', _lib.ptr(u), _lib.ptr(d), B, L, D, nl, dims_c, ptrs(ks), ptrs(bs), ctx.act, _lib.ptr(dmat),
                  _lib.ptr(dsum), _lib.ptr(du), _lib.ptr(dd), ptrs(dks), ptrs(dbs), _lib.ptr(ws), ws.numel(), _lib.stream())
        return (du, dd, None, None, *dks, *dbs)


class DinAttention(Layer):
    """The weights of attention_by_dnn: Dense layers `layer{i}` (kernel (in, out), bias (out,)), the first taking [user | doc] (2D).

    Unlike the reference's keras.Sequential, which maps the concatenated (B, L, 2D) input to logits, calling this module runs the
    whole attention unit: `model(user_emb, doc_emb)` returns (attn_mat (B, D), attn_score_sum (B, 1)) with these weights, on one
    fused HIP kernel per direction (csrc/attention_dnn.hip).  It builds lazily from the first user_emb's D."""

    def __init__(self, dnn_dims, dnn_activation='relu', **kwargs):
        super().__init__(**kwargs)
        dims = [int(v) for v in dnn_dims]
        if not dims or any(v < 1 for v in dims):
            raise ValueError('dnn_dims must be a non-empty list of positive widths, got %r' % (list(dnn_dims),))
        if dims[-1] != 1:
            raise ValueError('the last of dnn_dims must be 1 (the attention logit), got %r' % (dims,))
        if len(dims) - 1 > _DIN_MAX_HIDDEN:
            raise NotImplementedError('attention_by_dnn kernels cover at most %d hidden layers (the reference has no limit); got %d'
                                      % (_DIN_MAX_HIDDEN, len(dims) - 1))
        if max(dims) > _DIN_MAX_WIDTH:
            raise NotImplementedError('attention_by_dnn kernels cover Dense widths <= %d (the reference has no limit); got %r'
                                      % (_DIN_MAX_WIDTH, dims))
        code, fn = activation_code(dnn_activation)
        if fn is not None:
            raise NotImplementedError('attention_by_dnn fuses the activations linear, relu, tanh and sigmoid between its Dense layers; '
                                      'a callable activation (%r) cannot run inside the fused kernel' % (dnn_activation,))
        self.dnn_dims = dims
        self.dnn_activation = dnn_activation
        self.act_code = code

    def build(self, input_shape):
        """Creates `layer{i}/kernel` (in, dims[i]) and `layer{i}/bias` (dims[i],): glorot_uniform and zeros, as keras.layers.Dense."""
        D = int(input_shape[0][-1]) if isinstance(input_shape[0], (list, tuple)) else int(input_shape[-1])
        if D > _DIN_MAX_WIDTH:
            raise NotImplementedError('attention_by_dnn kernels cover embedding_dim <= %d (the reference has no limit); got %d'
                                      % (_DIN_MAX_WIDTH, D))
        self.embedding_dim = D
        self.kernels, self.biases = [], []
        width = 2 * D
        for i, dim in enumerate(self.dnn_dims):
            self.kernels.append(self.add_weight('layer%d/kernel' % i, shape=[width, dim], initializer='glorot_uniform'))
            self.biases.append(self.add_weight('layer%d/bias' % i, shape=[dim], initializer='zeros'))
            width = dim
        self.built = True

    def forward(self, user_emb, doc_emb):
        for t, what, nd in ((user_emb, 'user_emb', 3), (doc_emb, 'doc_emb', 2)):
            if not isinstance(t, torch.Tensor):
                raise TypeError('%s must be a torch.Tensor, got %s' % (what, type(t)))
            if t.dim() != nd:
                raise ValueError('user_emb must be (B, L, D) and doc_emb (B, D); got %s and %s'
                                 % (tuple(user_emb.shape), tuple(doc_emb.shape)))
        if user_emb.shape[0] != doc_emb.shape[0] or user_emb.shape[2] != doc_emb.shape[1]:
            raise ValueError('user_emb must be (B, L, D) and doc_emb (B, D); got %s and %s' % (tuple(user_emb.shape), tuple(doc_emb.shape)))
        if not self.built:
            self._build_device = user_emb.device
            self.build((tuple(user_emb.shape), tuple(doc_emb.shape)))
        if user_emb.shape[2] != self.embedding_dim:
            raise ValueError('this attention model was built for embedding_dim %d, got %d' % (self.embedding_dim, user_emb.shape[2]))
        return self.call(user_emb, doc_emb)

    def call(self, user_emb, doc_emb):
        _lib.require_gpu(user_emb, 'user_emb')
        _lib.require_gpu(doc_emb, 'doc_emb')
        return _AttnDnnFunction.apply(user_emb, doc_emb, tuple(self.dnn_dims), self.act_code, *self.kernels, *self.biases)


def attention_by_dnn(user_emb, doc_emb, dnn_dims, dnn_activation='relu', dnn_name='din'):
    """DIN attention: a Dense stack scores each of the L user embeddings against the item embedding.

    Args:
        user_emb: (B, L, D);  doc_emb: (B, D);
        dnn_dims: widths of the Dense layers; a 1 is appended to this list when its last entry is not 1 (as the reference does);
        dnn_activation: 'relu' (default), 'tanh', 'sigmoid', 'linear' or None, on every Dense layer but the last;
        dnn_name: name of the returned model (its weights are `layer{i}/kernel`, `layer{i}/bias`).
    Returns:
        attn_mat (B, D) = sum_l sigmoid(logit_l) user_emb[:, l],  attn_score_sum (B, 1) = sum_l sigmoid(logit_l),  and the model
        (a DinAttention: `model(user_emb, doc_emb)` recomputes both outputs with the same weights).
    Limits of the fused kernels (NotImplementedError): D and every width <= 256, at most 3 hidden layers, a named activation.
    """
    if dnn_dims[-1] != 1:
        dnn_dims.append(1)
    model = DinAttention(dnn_dims, dnn_activation=dnn_activation, name=dnn_name)
    attn_mat, attn_score_sum = model(user_emb, doc_emb)
    return attn_mat, attn_score_sum, model


_SOFTMAX_MAX_D = 256                                     # AS_MAX_D / AS_MAX_H of csrc/attention_softmax.hip
_SOFTMAX_MAX_H = 8
_LN2 = math.log(2.0)


def attention_softmax_supported(L, D, H):
    """Whether the kernels take this shape (host-only query of the library, no device call)."""
    return bool(_lib.load().recnow_attention_softmax_supported(int(L), int(D), int(H)))


class _AttnSoftmaxFunction(torch.autograd.Function):
    """(user_emb (B, L, D), query (B, H, D), lengths (B,) int32 | None, mask (B, L) uint8 | None, scale) -> out (B, H, D), stat (B, H, 2).
    stat = (maximum, log2 of the sum rescaled by it) per (b, h): what the backward recomputes the weights from.  Saves its inputs, out and
    stat; nothing of size B H L exists in either direction."""

    @staticmethod
    def forward(ctx, user_emb, query, lengths, mask, scale):
        u = _lib.f32c(user_emb, 'user_emb')
        q = _lib.f32c(query, 'query')
        B, L, D = u.shape
        H = q.shape[1]
        if B == 0 or L == 0:                               # nothing to launch: no key anywhere
            out = torch.zeros((B, H, D), dtype=torch.float32, device=u.device)
            stat = torch.full((B, H, 2), float('-inf'), dtype=torch.float32, device=u.device)
        else:
            out = torch.empty((B, H, D), dtype=torch.float32, device=u.device)
            stat = torch.empty((B, H, 2), dtype=torch.float32, device=u.device)
            _lib.call('recnow_attention_softmax_fwd', _lib.ptr(u), _lib.ptr(q), _lib.ptr(lengths), _lib.ptr(mask), B, L, D, H, scale,
                      _lib.ptr(out), _lib.ptr(stat), _lib.stream())
        ctx.save_for_backward(u, q, out, stat)
        ctx.keys = (lengths, mask)
        ctx.scale = scale
        ctx.mark_non_differentiable(stat)
        ctx.set_materialize_grads(False)                   # no zeros tensor for the statistic's absent gradient
        return out, stat

    @staticmethod
    def backward(ctx, dout, _dstat):
        u, q, out, stat = ctx.saved_tensors
        lengths, mask = ctx.keys
        B, L, D = u.shape
        H = q.shape[1]
        need_u, need_q = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if dout is None:
            return None, None, None, None, None
        if B == 0 or L == 0:
            return (torch.zeros_like(u) if need_u else None, torch.zeros_like(q) if need_q else None, None, None, None)
        du = torch.empty_like(u) if need_u else None       # every row is written by the kernel
        dq = torch.empty_like(q) if need_q else None
        if need_u or need_q:
            dout = _lib.f32c(dout, 'grad')
            _lib.call('recnow_attention_softmax_bwd', _lib.ptr(u), _lib.ptr(q), _lib.ptr(lengths), _lib.ptr(mask), _lib.ptr(out), _lib.ptr(stat),
                      _lib.ptr(dout), B, L, D, H, ctx.scale, _lib.ptr(du), _lib.ptr(dq), _lib.stream())
        return du, dq, None, None, None


def attention_by_softmax(user_emb, query, lengths=None, mask=None, scale=None, return_lse=False):
    """Masked multi-head softmax target attention: the candidate item is the query, the L history positions are keys and values.

    Args:
        user_emb: (B, L, D) float32 GPU tensor, the keys and also the values;
        query: (B, D) for one head or (B, H, D) for H heads;
        lengths: (B,) or (B, 1) integers, position l of sample b is a key iff l < lengths[b] (above L acts as L, negative as 0);
        mask: (B, L) of any integer, bool or float dtype, non-zero = key; with lengths too, the two are ANDed; neither: every position is a key;
        scale: a finite float > 0, None = 1 / sqrt(D);
        return_lse: also return lse = log sum_{keys} exp(score), (B, H) or (B,), not differentiable.
    Returns:
        out[b, h] = sum_l softmax_l(scale <query[b, h], user_emb[b, l]>) user_emb[b, l] over the keys: (B, H, D), or (B, D) for a 2-D query.
        A sample without a key gets out = 0 and lse = -inf and contributes nothing to any gradient; positions that are not keys may hold
        NaN or inf, their d user_emb rows are 0.
    Limits of the fused kernels (NotImplementedError): D <= 256, H <= 8.  One HIP kernel per direction (csrc/attention_softmax.hip), no
    host synchronisation, no atomics; the backward recomputes the scores from the inputs and a per-(b, h) (maximum, log-sum) pair.
    """
    for t, what in ((user_emb, 'user_emb'), (query, 'query')):
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s must be a torch.Tensor, got %s' % (what, type(t)))
    if user_emb.dim() != 3 or query.dim() not in (2, 3):
        raise ValueError('user_emb must be (B, L, D) and query (B, D) or (B, H, D); got %s and %s' % (tuple(user_emb.shape), tuple(query.shape)))
    B, L, D = user_emb.shape
    two_d = query.dim() == 2
    H = 1 if two_d else query.shape[1]
    if query.shape[0] != B or query.shape[-1] != D or H < 1 or D < 1:
        raise ValueError('user_emb must be (B, L, D) and query (B, D) or (B, H, D) with the same B and D >= 1, H >= 1; got %s and %s'
                         % (tuple(user_emb.shape), tuple(query.shape)))
    if lengths is not None:
        if not isinstance(lengths, torch.Tensor):
            raise TypeError('lengths must be a torch.Tensor, got %s' % type(lengths))
        if lengths.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
            raise ValueError('lengths must be integers (int32 or int64), got %s' % lengths.dtype)
        if lengths.numel() != B or lengths.dim() not in (1, 2):
            raise ValueError('lengths must be (B,) or (B, 1) with B = %d; got %s' % (B, tuple(lengths.shape)))
    if mask is not None:
        if not isinstance(mask, torch.Tensor):
            raise TypeError('mask must be a torch.Tensor, got %s' % type(mask))
        if mask.dim() != 2 or mask.shape[0] != B or mask.shape[1] != L or mask.dtype.is_complex:
            raise ValueError('mask must be (B, L) = (%d, %d); got %s' % (B, L, tuple(mask.shape)))
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    scale = float(scale)
    if not (math.isfinite(scale) and scale > 0.0):
        raise ValueError('scale must be a finite float > 0, got %r' % (scale,))
    if D > _SOFTMAX_MAX_D:
        raise NotImplementedError('attention_by_softmax kernels cover embedding_dim <= %d; got %d' % (_SOFTMAX_MAX_D, D))
    if H > _SOFTMAX_MAX_H:
        raise NotImplementedError('attention_by_softmax kernels cover at most %d heads; got %d' % (_SOFTMAX_MAX_H, H))
    _lib.require_gpu(user_emb, 'user_emb')                 # after the argument checks: those hold on any device
    _lib.require_gpu(query, 'query')
    if lengths is not None:
        _lib.require_gpu(lengths, 'lengths')
        lengths = lengths.reshape(-1)
        if lengths.dtype != torch.int32:
            lengths = lengths.clamp(0, L).to(torch.int32)  # before the narrowing: an int64 above 2^31 acts as L
        lengths = lengths.contiguous()
    if mask is not None:
        _lib.require_gpu(mask, 'mask')
        if mask.dtype not in (torch.uint8, torch.bool):
            mask = mask != 0
        mask = mask.contiguous()
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
    out, stat = _AttnSoftmaxFunction.apply(user_emb, query.unsqueeze(1) if two_d else query, lengths, mask, scale)
    if two_d:
        out = out.reshape(B, D)
    if not return_lse:
        return out
    lse = (stat[..., 0].double() + stat[..., 1].double() * _LN2).to(torch.float32)     # -inf for a sample without a key
    return out, (lse.reshape(B) if two_d else lse)
