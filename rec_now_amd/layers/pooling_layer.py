"""PoolingLayer -- drop-in for rec_now/layers/pooling_layer.py: reduce a tensor over an axis with 'sum', 'mean', 'max' or 'min'
(tf.reduce_sum / reduce_mean / reduce_max / reduce_min).  Host side of the reduction kernels of csrc/tensor_util.hip.

The contiguous input is folded to (O, R, I) -- the extents before, of and after the reduced axes -- and one launch reduces over R (two for one
long row, e.g. axis=None).  No host synchronisation, no float atomics: the same input gives the same bits on every run, forward and backward.
The gradient of 'max' / 'min' follows TensorFlow: every position equal to the result receives g / count, count being the number of such
positions of that run.
"""
import torch

from .. import _lib
from ._keras import Layer

_OPS = {'sum': 0, 'mean': 1, 'max': 2, 'min': 3}          # RECNOW_REDUCE_* of include/recnow.h


def _fold(shape, axis):
    """(normalised axes, O, R, I) of reducing `axis` (int, None or a sequence that forms one contiguous run of axes) of a tensor of `shape`."""
    rank = len(shape)
    if axis is None:
        axes = list(range(rank))
    else:
        listed = isinstance(axis, (list, tuple))
        raw = [int(a) for a in axis] if listed else [int(axis)]
        axes = []
        for a in raw:
            if a < -rank or a >= rank:
                raise ValueError('axis %d is out of range for a tensor of rank %d' % (a, rank))
            axes.append(a % rank)
        axes = sorted(axes)
        if len(set(axes)) != len(axes) or (axes and axes[-1] - axes[0] + 1 != len(axes)):
            raise NotImplementedError('PoolingLayer reduces one axis or one contiguous run of axes; axes %s are not one' % (list(axis),))
    O = R = I = 1
    for d, n in enumerate(shape):
        if d in axes:
            R *= int(n)
        elif not axes or d < axes[0]:
            O *= int(n)
        else:
            I *= int(n)
    return axes, O, R, I


class _ReduceFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, op, O, R, I, out_shape):
        out = torch.empty(out_shape, dtype=torch.float32, device=x.device)            # every element is written by the kernel
        if O * I > 0:
            nws = _lib.load().recnow_reduce_axis_workspace_bytes(O, R, I)
            ws = _lib.workspace(nws, x.device) if nws else None
            _lib.call('recnow_reduce_axis_fwd', _lib.ptr(x), O, R, I, op, _lib.ptr(out), _lib.ptr(ws), nws, _lib.stream())
        if op >= _OPS['max']:
            ctx.save_for_backward(x, out)
        ctx.meta = (op, O, R, I, tuple(x.shape))
        return out

    @staticmethod
    def backward(ctx, g):
        op, O, R, I, shape = ctx.meta
        x, y = ctx.saved_tensors if op >= _OPS['max'] else (None, None)
        g = _lib.f32c(g, 'grad')
        dx = torch.empty(shape, dtype=torch.float32, device=g.device)
        _lib.call('recnow_reduce_axis_bwd', _lib.ptr(x), _lib.ptr(y), _lib.ptr(g), O, R, I, op, _lib.ptr(dx), _lib.stream())
        return dx, None, None, None, None, None


def _reduce(inputs, axis, keepdims, combiner):
    if not isinstance(inputs, torch.Tensor):
        raise TypeError('inputs must be a torch.Tensor, got %s' % type(inputs))
    if inputs.dtype != torch.float32:
        raise TypeError('PoolingLayer reduces float32 tensors, got %s' % inputs.dtype)
    shape = tuple(inputs.shape)
    axes, O, R, I = _fold(shape, axis)
    if R == 0:
        raise ValueError("cannot reduce over an empty axis (shape %s, axis %r) with '%s'" % (shape, axis, combiner))
    _lib.require_gpu(inputs, 'inputs')                 # after the argument checks: those hold on any device
    if keepdims:
        out_shape = tuple(1 if d in axes else n for d, n in enumerate(shape))
    else:
        out_shape = tuple(n for d, n in enumerate(shape) if d not in axes)
    return _ReduceFunction.apply(inputs.contiguous(), _OPS[combiner], O, R, I, out_shape)


def reduce_mean(inputs, axis=None, keepdims=False):
    return _reduce(inputs, axis, keepdims, 'mean')


def reduce_sum(inputs, axis=None, keepdims=False):
    return _reduce(inputs, axis, keepdims, 'sum')


def reduce_max(inputs, axis=None, keepdims=False):
    return _reduce(inputs, axis, keepdims, 'max')


def reduce_min(inputs, axis=None, keepdims=False):
    return _reduce(inputs, axis, keepdims, 'min')


class PoolingLayer(Layer):
    """Reduce the input over `axis`.

    Example:
        inputs = [[1, 2, 3], [10, 11, 12]]
        PoolingLayer(axis=0, keepdims=True, combiner='sum')(inputs) = [[11, 13, 15]]
        PoolingLayer(axis=1, keepdims=False, combiner='sum')(inputs) = [6, 33]
    """
    combiner_to_func = {
        'mean': reduce_mean,
        'sum': reduce_sum,
        'max': reduce_max,
        'min': reduce_min,
    }

    def __init__(self, axis=None, keepdims=False, combiner=None, name=None, **kwargs):
        """
        Args:
            axis: the axis to reduce: an int (negative counts from the end), None (all elements: a scalar, or an all-ones shape with
                keepdims), or a sequence of ints that forms one contiguous run of axes (any other sequence: NotImplementedError).
            keepdims: keep the reduced axes with length 1.
            combiner: None (the input is returned), 'mean', 'sum', 'max', 'min', or a callable (called on the input).
            name: the layer's name.
        """
        super().__init__(name=name, **kwargs)
        self.axis = axis
        self.keepdims = keepdims
        self.combiner = combiner

    def call(self, inputs):
        """float32 GPU tensor of any rank (made contiguous if it is not) -> its reduction.  An empty reduced axis raises ValueError."""
        combiner = self.combiner
        if combiner is None:
            return inputs
        if callable(combiner):
            return combiner(inputs)
        if combiner in PoolingLayer.combiner_to_func:
            return PoolingLayer.combiner_to_func[combiner](inputs, axis=self.axis, keepdims=self.keepdims)
        raise ValueError("combiner must be one of None, "
                         "'mean', 'sum', 'max', 'min' or a callable object")
