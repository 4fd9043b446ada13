"""BilinearInteractionLayer -- the bilinear cross of FiBiNET (Huang, Zhang and Zhang 2019, arXiv 1905.09433, section 3.3); the
reference package has no such layer, this module is the definition.

The F field embeddings of a sample interact pair by pair through a learned (D, D) matrix:

    p_ij = (v_i W) * v_j          for the P = F(F-1)/2 pairs i < j, in InnerPNNLayer's i-major order

with one matrix for every pair ('all'), one per left field ('each') or one per pair ('interaction').  One HIP kernel per direction
(csrc/bilinear.hip) keeps the projection U = X W on chip; the backward recomputes it, so the layer saves its inputs and allocates its
output, its gradients and (for the weight gradient only) the workspace the library asks for.

Symbols: B batch size, D embedding dim, F number of fields, P = F(F-1)/2.
"""
import torch

from .. import _lib
from ._fields import check_fields
from ._keras import Layer, get_initializer

_TYPES = {'all': 0, 'each': 1, 'interaction': 2}        # RECNOW_BILINEAR_* of include/recnow.h
_MAX_F, _MAX_D = 64, 64                                  # BIL_MAX_F, BIL_MAX_D of csrc/bilinear.hip


def n_weights(bilinear_type, F):
    """Matrices in `bilinear_weight` for F fields: 1, max(F-1, 1) or max(P, 1)."""
    if bilinear_type == 'all':
        return 1
    if bilinear_type == 'each':
        return max(F - 1, 1)
    return max(F * (F - 1) // 2, 1)


def bilinear_supported(F, D, bilinear_type='interaction'):
    """Whether the kernels take this shape (host-only query of the library, no device call)."""
    return bool(_lib.load().recnow_bilinear_supported(int(F), int(D), _TYPES[bilinear_type]))


class _BilinearFunction(torch.autograd.Function):
    """(W (nW, D, D), x_0 .. x_{F-1} (B, D)) -> (B, P*D).  Saves its inputs; the backward kernels recompute U = X W."""

    @staticmethod
    def forward(ctx, kind, weight, *fields):
        xs = [_lib.f32c(x, 'BilinearInteraction input') for x in fields]
        w = _lib.f32c(weight, 'bilinear_weight')
        B, D = xs[0].shape
        F = len(xs)
        dev = xs[0].device
        out = torch.empty((B, F * (F - 1) // 2 * D), dtype=torch.float32, device=dev)
        if out.numel() > 0:
            ptrs = _lib.ptr_array(xs, dev)
            _lib.call('recnow_bilinear_fwd', _lib.ptr(ptrs), F, B, D, kind, _lib.ptr(w), _lib.ptr(out), _lib.stream())
        ctx.save_for_backward(w, *xs)
        ctx.kind = kind
        return out

    @staticmethod
    def backward(ctx, dout):
        w, xs = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        kind, F = ctx.kind, len(xs)
        B, D = xs[0].shape
        dev = xs[0].device
        need_w = ctx.needs_input_grad[1]
        if B == 0 or F == 1:                                 # no pair: nothing depends on the inputs
            return (None, torch.zeros_like(w) if need_w else None) + tuple(torch.zeros_like(x) for x in xs)
        dout = _lib.f32c(dout, 'grad')
        dx = torch.empty((F, B, D), dtype=torch.float32, device=dev)         # every row is written by the kernel
        dw = ws = None
        ws_bytes = 0
        if need_w:
            dw = torch.empty_like(w)
            ws_bytes = int(_lib.load().recnow_bilinear_workspace_bytes(B, F, D, kind))
            ws = _lib.workspace(ws_bytes, dev)
        _lib.call('recnow_bilinear_bwd', _lib.ptr(_lib.ptr_array(list(xs), dev)), _lib.ptr(_lib.block_ptr_array(dx, F)), F, B, D, kind,
                  _lib.ptr(w), _lib.ptr(dout), _lib.ptr(dw), _lib.ptr(ws), ws_bytes, _lib.stream())
        return (None, dw) + tuple(dx.unbind(0))


class BilinearInteractionLayer(Layer):
    """FiBiNET's bilinear interaction: block p of the output is (x_i @ W[w]) * x_j for the p-th pair i < j, with
    w = 0 ('all'), i ('each') or p ('interaction')."""

    def __init__(self, bilinear_type='interaction', kernel_initializer='glorot_uniform', kernel_regularizer=None, kernel_constraint=None,
                 **kwargs):
        """
        Args:
            bilinear_type: 'all' (one matrix), 'each' (one per left field, F-1) or 'interaction' (one per pair, P; the paper's best setting).
            kernel_initializer: a name of _keras.get_initializer, drawn per (D, D) matrix (Glorot fans are D and D), or a callable that is
                handed the full (nW, D, D) shape.
            kernel_regularizer, kernel_constraint: kept with the weight, as add_weight does.
        """
        super().__init__(**kwargs)
        if bilinear_type not in _TYPES:
            raise ValueError("bilinear_type must be one of 'all', 'each', 'interaction'; got %r" % (bilinear_type,))
        self.bilinear_type = bilinear_type
        self.kernel_initializer = kernel_initializer
        self.kernel_regularizer = kernel_regularizer
        self.kernel_constraint = kernel_constraint

    def build(self, input_shape):
        F, D = check_fields('BilinearInteractionLayer', input_shape, allow_3d=False)
        nW = n_weights(self.bilinear_type, F)
        init = self.kernel_initializer
        if not callable(init):
            one = get_initializer(init)                       # per matrix: the fans of a (D, D) kernel, not of the stack
            init = lambda shape: torch.stack([one((D, D)) for _ in range(nW)])      # noqa: E731
        self.bilinear_weight = self.add_weight('bilinear_weight', (nW, D, D), initializer=init, regularizer=self.kernel_regularizer,
                                               constraint=self.kernel_constraint)
        self.built = True

    def call(self, inputs):
        """inputs: list of F float32 GPU tensors of shape (B, D).  Returns (B, P*D), block p at columns [p*D, (p+1)*D)."""
        F, D = check_fields('BilinearInteractionLayer', [tuple(x.shape) for x in inputs], allow_3d=False)
        w = self.bilinear_weight
        if tuple(w.shape) != (n_weights(self.bilinear_type, F), D, D):
            raise ValueError("bilinear_weight has shape %s; bilinear_type '%s' with %d fields of width %d needs %s"
                             % (tuple(w.shape), self.bilinear_type, F, D, (n_weights(self.bilinear_type, F), D, D)))
        if F > _MAX_F or D > _MAX_D:
            raise NotImplementedError('BilinearInteractionLayer kernels cover at most %d fields of embedding_dim <= %d; got %d fields of width %d'
                                      % (_MAX_F, _MAX_D, F, D))
        for x in inputs:
            _lib.require_gpu(x, 'BilinearInteraction input')          # after the argument checks: those hold on any device
        return _BilinearFunction.apply(_TYPES[self.bilinear_type], w, *inputs)
