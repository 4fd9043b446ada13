"""InteractingLayer -- the multi-head self-attention over the fields of AutoInt (Song et al. 2019, arXiv 1810.11921, section 4.3; DeepCTR's
layer of the same name); the reference package has no such layer, this module is the definition.

A sample has F fields x_f of width D; H heads of width d, E = H d; weights W_query, W_key, W_value (and W_res with use_res), each (D, E):

    Q = X W_query, K = X W_key, V = X W_value             (F, E); head h is columns [h d, (h+1) d)
    S_h = Q_h K_h^T                                       (F, F); times 1/sqrt(d) with scaling=True
    A_h = softmax of S_h over the keys (row maximum subtracted),   O_h = A_h V_h
    pre = concat_h O_h (+ X W_res),   out = relu(pre)  (activation='relu')  or  pre  (activation=None)

The ReLU subgradient at 0 is 0.  One HIP kernel per direction (csrc/autoint.hip) keeps Q, K, V, S, A and pre on chip; the backward recomputes
them, so the layer saves its inputs and allocates its output, its gradients and (for the weight gradients only) the workspace the library asks
for.  No host synchronisation: the layer can be captured in a HIP graph.

Symbols: B batch size, F number of fields, D embedding dim, H head_num, d att_embedding_size, E = H d.
"""
import torch

from .. import _lib
from ._fields import check_fields, field_table, rows_table
from ._keras import Layer, get_initializer

_MAX_F, _MAX_D, _MAX_E, _MAX_H = 64, 64, 64, 8           # AI_MAX_* of csrc/autoint.hip
_ACTIVATIONS = {'relu': 1, None: 0}


def autoint_supported(F, D, head_num, att_embedding_size):
    """Whether the kernels take this shape (host-only query of the library, no device call)."""
    return bool(_lib.load().recnow_autoint_supported(int(F), int(D), int(head_num), int(att_embedding_size)))


class _InteractingFunction(torch.autograd.Function):
    """(cfg, W_query, W_key, W_value, W_res or None, x (B, F, D) | x_0 .. x_{F-1} (B, D)) -> (B, F, E) | (B, F*E).  Saves its inputs."""

    @staticmethod
    def forward(ctx, cfg, wq, wk, wv, wr, *inputs):
        H, d, scaling, relu = cfg
        three_d = inputs[0].dim() == 3
        if three_d:
            x = _lib.f32c(inputs[0], 'InteractingLayer input')
            B, F, D = x.shape
            xs = [x]
            table, stride = rows_table(x), F * D
        else:
            for t in inputs:
                _lib.require_gpu(t, 'InteractingLayer input')
            xs, table, stride = field_table(list(inputs), 'InteractingLayer input')
            B, D = xs[0].shape
            F = len(xs)
        ws = [_lib.f32c(w, 'InteractingLayer weight') if w is not None else None for w in (wq, wk, wv, wr)]
        E = H * d
        dev = xs[0].device
        out = torch.empty((B, F, E) if three_d else (B, F * E), dtype=torch.float32, device=dev)
        if B > 0:
            _lib.call('recnow_autoint_fwd', _lib.ptr(table), stride, F, B, D, H, d, _lib.ptr(ws[0]), _lib.ptr(ws[1]), _lib.ptr(ws[2]),
                      _lib.ptr(ws[3]), scaling, relu, _lib.ptr(out), _lib.stream())
        ctx.save_for_backward(*([w for w in ws if w is not None] + xs))
        ctx.cfg, ctx.three_d, ctx.table, ctx.stride, ctx.dims, ctx.nW = cfg, three_d, table, stride, (B, F, D), 3 + (wr is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        H, d, scaling, relu = ctx.cfg
        B, F, D = ctx.dims
        nW = ctx.nW
        ws = list(ctx.saved_tensors[:nW]) + [None] * (4 - nW)
        dev = dout.device
        need_w = any(ctx.needs_input_grad[1:1 + nW])
        dx = torch.empty((B, F, D), dtype=torch.float32, device=dev)          # every row is written by the kernel
        dws = [None] * 4
        if B == 0:
            dws = [torch.zeros_like(w) if need_w and w is not None else None for w in ws]
        else:
            dout = _lib.f32c(dout, 'grad')
            wsp, ws_bytes = None, 0
            if need_w:
                dws = [torch.empty_like(w) if w is not None else None for w in ws]
                ws_bytes = int(_lib.load().recnow_autoint_workspace_bytes(B, F, D, H, d, int(nW == 4)))
                wsp = _lib.workspace(ws_bytes, dev)
            _lib.call('recnow_autoint_bwd', _lib.ptr(ctx.table), ctx.stride, _lib.ptr(rows_table(dx)), F * D, F, B, D, H, d, _lib.ptr(ws[0]),
                      _lib.ptr(ws[1]), _lib.ptr(ws[2]), _lib.ptr(ws[3]), scaling, relu, _lib.ptr(dout), _lib.ptr(dws[0]), _lib.ptr(dws[1]),
                      _lib.ptr(dws[2]), _lib.ptr(dws[3]), _lib.ptr(wsp), ws_bytes, _lib.stream())
        grads = (dx,) if ctx.three_d else tuple(dx[:, f] for f in range(F))
        return (None, dws[0], dws[1], dws[2], dws[3]) + grads


class InteractingLayer(Layer):
    """AutoInt's interacting layer: multi-head self-attention over the F fields of a sample, with an optional residual projection and ReLU."""

    def __init__(self, att_embedding_size=8, head_num=2, use_res=True, scaling=False, activation='relu', kernel_initializer='glorot_uniform',
                 kernel_regularizer=None, kernel_constraint=None, **kwargs):
        """
        Args:
            att_embedding_size: d, the width of one head.
            head_num: H; the output width per field is E = H d.
            use_res: add the residual projection X W_res.
            scaling: multiply the scores by 1/sqrt(d).
            activation: 'relu' or None.
            kernel_initializer: a name of _keras.get_initializer or a callable, drawn per (D, E) matrix (Glorot fans are D and E).
            kernel_regularizer, kernel_constraint: kept with every weight, as add_weight does.
        """
        super().__init__(**kwargs)
        if int(head_num) < 1:
            raise ValueError('head_num must be >= 1, got %r' % (head_num,))
        if int(att_embedding_size) < 1:
            raise ValueError('att_embedding_size must be >= 1, got %r' % (att_embedding_size,))
        if activation not in _ACTIVATIONS:
            raise ValueError("activation must be 'relu' or None, got %r" % (activation,))
        self.att_embedding_size = int(att_embedding_size)
        self.head_num = int(head_num)
        self.use_res = bool(use_res)
        self.scaling = bool(scaling)
        self.activation = activation
        self.kernel_initializer = kernel_initializer
        self.kernel_regularizer = kernel_regularizer
        self.kernel_constraint = kernel_constraint

    def build(self, input_shape):
        F, D = check_fields('InteractingLayer', input_shape)
        E = self.head_num * self.att_embedding_size
        for name in ('W_query', 'W_key', 'W_value') + (('W_res',) if self.use_res else ()):
            w = self.add_weight(name, (D, E), initializer=get_initializer(self.kernel_initializer), regularizer=self.kernel_regularizer,
                                constraint=self.kernel_constraint)
            setattr(self, name, w)
        if not self.use_res:
            self.W_res = None
        self.built = True

    def call(self, inputs):
        """inputs: a float32 GPU tensor (B, F, D) -> (B, F, E), or a list of F float32 GPU tensors (B, D) -> (B, F*E), block f at
        columns [f E, (f+1) E)."""
        if isinstance(inputs, torch.Tensor):
            F, D = check_fields('InteractingLayer', tuple(inputs.shape))
            tensors = [inputs]
        else:
            if not isinstance(inputs, (list, tuple)) or len(inputs) < 1:
                raise ValueError('InteractingLayer takes a (B, F, D) tensor or a list of (B, D) field tensors')
            F, D = check_fields('InteractingLayer', [tuple(x.shape) for x in inputs])
            tensors = list(inputs)
        H, d = self.head_num, self.att_embedding_size
        E = H * d
        for name in ('W_query', 'W_key', 'W_value') + (('W_res',) if self.use_res else ()):
            if tuple(getattr(self, name).shape) != (D, E):
                raise ValueError('%s has shape %s; fields of width %d with %d heads of width %d need %s'
                                 % (name, tuple(getattr(self, name).shape), D, H, d, (D, E)))
        if F > _MAX_F or D > _MAX_D or E > _MAX_E or H > _MAX_H:
            raise NotImplementedError('InteractingLayer kernels cover at most %d fields, embedding_dim <= %d, head_num * att_embedding_size <= %d '
                                      'and head_num <= %d; got F = %d, D = %d, E = %d, H = %d' % (_MAX_F, _MAX_D, _MAX_E, _MAX_H, F, D, E, H))
        for x in tensors:
            _lib.require_gpu(x, 'InteractingLayer input')             # after the argument checks: those hold on any device
        cfg = (H, d, int(self.scaling), _ACTIVATIONS[self.activation])
        return _InteractingFunction.apply(cfg, self.W_query, self.W_key, self.W_value, self.W_res, *tensors)
