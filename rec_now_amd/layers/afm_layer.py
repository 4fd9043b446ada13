"""AFMLayer -- the attention-pooled pairwise interaction of the Attentional Factorization Machine (Xiao et al. 2017, arXiv 1708.04617,
section 3; DeepCTR's layer of the same name); the reference package has no such layer, this module is the definition.

A sample has F fields x_f of width D; A = attention_factor; weights attention_W (D, A), attention_b (A,), projection_h (A, 1) and, with
projection=True, projection_p (D, 1).  Over the P = F (F - 1) / 2 pairs k = (i, j), i < j, in InnerPNN's i-major order:

    p_k = x_i * x_j                                        (D)
    z_k = attention_W^T p_k + attention_b,   e_k = <relu(z_k), projection_h>
    a   = softmax of e over the pairs (maximum subtracted),   v = sum_k a_k p_k      (D)
    out = <v, projection_p>  (B, 1)  with projection=True,   v  (B, D)  with projection=False

The ReLU subgradient at 0 is 0.  One HIP kernel per direction (csrc/afm.hip) keeps the pair products, the hidden layer and the attention on
chip; the backward recomputes them, so the layer saves its inputs and allocates its output, its gradients and (for the weight gradients only)
the workspace the library asks for.  No host synchronisation: the layer can be captured in a HIP graph.  DeepCTR's dropout on v
(`dropout_rate`) is not built.  A single field has no pair: the output and every gradient are zeros, and the library is not called.

Symbols: B batch size, F number of fields, D embedding dim, A attention_factor, P number of pairs.
"""
import torch

from .. import _lib
from ._keras import Layer, get_initializer
from ._fields import check_fields, field_table, rows_table

_MAX_F, _MAX_D, _MAX_A = 64, 64, 64                      # AFM_MAX_* of csrc/afm.hip


def afm_supported(F, D, attention_factor):
    """Whether the kernels take this shape (host-only query of the library, no device call)."""
    return bool(_lib.load().recnow_afm_supported(int(F), int(D), int(attention_factor)))


class _AFMFunction(torch.autograd.Function):
    """(attention_W, attention_b, projection_h, projection_p or None, x (B, F, D) | x_0 .. x_{F-1} (B, D)) -> (B, 1) | (B, D).  Saves its inputs."""

    @staticmethod
    def forward(ctx, w, b, h, p, *inputs):
        three_d = inputs[0].dim() == 3
        if three_d:
            x = _lib.f32c(inputs[0], 'AFMLayer input')
            B, F, D = x.shape
            xs = [x]
            table, stride = rows_table(x), F * D
        else:
            for t in inputs:
                _lib.require_gpu(t, 'AFMLayer input')
            xs, table, stride = field_table(list(inputs), 'AFMLayer input')
            B, D = xs[0].shape
            F = len(xs)
        ws = [_lib.f32c(t, 'AFMLayer weight') if t is not None else None for t in (w, b, h, p)]
        A = ws[0].shape[1]
        dev = xs[0].device
        shape = (B, 1) if p is not None else (B, D)
        if F == 1:
            out = torch.zeros(shape, dtype=torch.float32, device=dev)
        else:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
            if B > 0:
                _lib.call('recnow_afm_fwd', _lib.ptr(table), stride, F, B, D, A, _lib.ptr(ws[0]), _lib.ptr(ws[1]), _lib.ptr(ws[2]), _lib.ptr(ws[3]),
                          _lib.ptr(out), _lib.stream())
        ctx.save_for_backward(*([t for t in ws if t is not None] + xs))
        ctx.three_d, ctx.table, ctx.stride, ctx.dims, ctx.nW = three_d, table, stride, (B, F, D, A), 3 + (p is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, F, D, A = ctx.dims
        nW = ctx.nW
        ws = list(ctx.saved_tensors[:nW]) + [None] * (4 - nW)
        dev = dout.device
        need_w = any(ctx.needs_input_grad[:nW])
        dws = [None] * 4
        if B == 0 or F == 1:
            dx = torch.zeros((B, F, D), dtype=torch.float32, device=dev)
            dws = [torch.zeros_like(t) if need_w and t is not None else None for t in ws]
        else:
            dx = torch.empty((B, F, D), dtype=torch.float32, device=dev)      # every row is written by the kernel
            dout = _lib.f32c(dout, 'grad')
            wsp, ws_bytes = None, 0
            if need_w:
                dws = [torch.empty_like(t) if t is not None else None for t in ws]
                ws_bytes = int(_lib.load().recnow_afm_workspace_bytes(B, F, D, A))
                wsp = _lib.workspace(ws_bytes, dev)
            _lib.call('recnow_afm_bwd', _lib.ptr(ctx.table), ctx.stride, _lib.ptr(rows_table(dx)), F * D, F, B, D, A, _lib.ptr(ws[0]), _lib.ptr(ws[1]),
                      _lib.ptr(ws[2]), _lib.ptr(ws[3]), _lib.ptr(dout), _lib.ptr(dws[0]), _lib.ptr(dws[1]), _lib.ptr(dws[2]), _lib.ptr(dws[3]),
                      _lib.ptr(wsp), ws_bytes, _lib.stream())
        grads = (dx,) if ctx.three_d else tuple(dx[:, f] for f in range(F))
        return (dws[0], dws[1], dws[2], dws[3]) + grads


class AFMLayer(Layer):
    """AFM's attention-based pooling of the pairwise interactions of the F fields of a sample.  DeepCTR's dropout on the pooled vector
    (`dropout_rate`) is not built."""

    def __init__(self, attention_factor=4, projection=True, kernel_initializer='glorot_normal', kernel_regularizer=None, kernel_constraint=None,
                 **kwargs):
        """
        Args:
            attention_factor: A, the width of the attention network's hidden layer.
            projection: project the pooled vector v (B, D) to a score (B, 1) with projection_p; False returns v and creates no projection_p.
            kernel_initializer: a name of _keras.get_initializer or a callable, drawn per matrix (attention_b starts at zeros).
            kernel_regularizer, kernel_constraint: kept with every matrix, as add_weight does.
        """
        super().__init__(**kwargs)
        if int(attention_factor) < 1:
            raise ValueError('attention_factor must be >= 1, got %r' % (attention_factor,))
        self.attention_factor = int(attention_factor)
        self.projection = bool(projection)
        self.kernel_initializer = kernel_initializer
        self.kernel_regularizer = kernel_regularizer
        self.kernel_constraint = kernel_constraint

    def build(self, input_shape):
        F, D = check_fields('AFMLayer', input_shape)
        A = self.attention_factor
        kw = dict(initializer=get_initializer(self.kernel_initializer), regularizer=self.kernel_regularizer, constraint=self.kernel_constraint)
        self.attention_W = self.add_weight('attention_W', (D, A), **kw)
        self.attention_b = self.add_weight('attention_b', (A,), initializer='zeros')
        self.projection_h = self.add_weight('projection_h', (A, 1), **kw)
        self.projection_p = self.add_weight('projection_p', (D, 1), **kw) if self.projection else None
        self.built = True

    def call(self, inputs):
        """inputs: a float32 GPU tensor (B, F, D) or a list of F float32 GPU tensors (B, D) -> (B, 1) with projection, else (B, D)."""
        if isinstance(inputs, torch.Tensor):
            F, D = check_fields('AFMLayer', tuple(inputs.shape))
            tensors = [inputs]
        else:
            if not isinstance(inputs, (list, tuple)) or len(inputs) < 1:
                raise ValueError('AFMLayer takes a (B, F, D) tensor or a list of (B, D) field tensors')
            F, D = check_fields('AFMLayer', [tuple(x.shape) for x in inputs])
            tensors = list(inputs)
        A = self.attention_factor
        want = [('attention_W', (D, A)), ('attention_b', (A,)), ('projection_h', (A, 1))] + ([('projection_p', (D, 1))] if self.projection else [])
        for name, shape in want:
            if tuple(getattr(self, name).shape) != shape:
                raise ValueError('%s has shape %s; fields of width %d with attention_factor %d need %s'
                                 % (name, tuple(getattr(self, name).shape), D, A, shape))
        if F > _MAX_F or D > _MAX_D or A > _MAX_A:
            raise NotImplementedError('AFMLayer kernels cover at most %d fields, embedding_dim <= %d and attention_factor <= %d; '
                                      'got F = %d, D = %d, A = %d' % (_MAX_F, _MAX_D, _MAX_A, F, D, A))
        for x in tensors:
            _lib.require_gpu(x, 'AFMLayer input')                      # after the argument checks: those hold on any device
        return _AFMFunction.apply(self.attention_W, self.attention_b, self.projection_h, self.projection_p, *tensors)
