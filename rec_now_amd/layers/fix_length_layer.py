"""pad_or_truncate / FixLengthLayer -- drop-in for rec_now/layers/fix_length_layer.py: cut an axis of a tensor to `length`, or fill it up at its end
with a constant.  It turns a ragged feature (a click history) into the fixed-length input a transformer or attention_by_dnn needs: for a
(batch_size, n, embedding_dim) tensor, pad_or_truncate(tensor, length, axis=1) has the shape (batch_size, length, embedding_dim).

Host side of k_pad_axis of csrc/tensor_util.hip: one launch that reads every kept element once and writes every output element once, for float32,
int32 and int64 tensors.  No host synchronisation.  The backward is the same kernel with the lengths exchanged and the constant 0.
"""
import struct

import torch

from .. import _lib
from ._keras import Layer

_PACK = {torch.float32: '<f', torch.int32: '<i', torch.int64: '<q'}


def _fill_bits(value, dtype):
    """The bit pattern of `value` as an element of `dtype`, in the low bytes of an int64 (recnow_pad_axis takes the element as bits)."""
    raw = struct.pack(_PACK[dtype], float(value) if dtype.is_floating_point else int(value))
    return struct.unpack('<q', raw.ljust(8, b'\0'))[0]


def _pad_launch(x, O, L_in, L_out, I, bits, out_shape):
    out = torch.empty(out_shape, dtype=x.dtype, device=x.device)                      # every element is written by the kernel
    _lib.call('recnow_pad_axis', _lib.ptr(x), x.element_size(), O, L_in, L_out, I, bits, _lib.ptr(out), _lib.stream())
    return out


class _PadFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, O, L_in, L_out, I, bits, out_shape):
        ctx.meta = (O, L_in, L_out, I, tuple(x.shape))
        out = _pad_launch(x, O, L_in, L_out, I, bits, out_shape)
        if not x.dtype.is_floating_point:
            ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, g):
        O, L_in, L_out, I, shape = ctx.meta
        return (_pad_launch(_lib.f32c(g, 'grad'), O, L_out, L_in, I, 0, shape),) + (None,) * 6


def pad_or_truncate(tensor, length, axis=-1, constant_values=0):
    """Cut the axis `axis` of `tensor` to `length`, or fill it up to `length` at its end with `constant_values`.

    A longer axis is truncated, a shorter one padded; an axis that already has the length returns `tensor` itself.

    Args:
        tensor: float32, int32 or int64 GPU tensor of any rank >= 1 (made contiguous if it is not).
        length (int): the length of the axis afterwards.
        axis (int, optional): the axis to cut or fill. Defaults to -1.
        constant_values (optional): the value that fills. Defaults to 0.

    Returns:
        The tensor with shape[axis] == length.  Float tensors carry a gradient (zero for nothing: the cut-off part gets zeros), integer ones none.
    """
    length = int(length)
    if not isinstance(tensor, torch.Tensor):
        raise TypeError('tensor must be a torch.Tensor, got %s' % type(tensor))
    if tensor.dtype not in _PACK:
        raise TypeError('pad_or_truncate takes float32, int32 and int64 tensors, got %s' % tensor.dtype)
    rank = tensor.dim()
    if rank < 1 or axis < -rank or axis >= rank:
        raise ValueError('axis %d is out of range for a tensor of rank %d' % (axis, rank))
    if length < 0:
        raise ValueError('length must be >= 0, got %d' % length)
    axis = axis % rank
    shape = tuple(tensor.shape)
    L_in = shape[axis]
    _lib.require_gpu(tensor, 'tensor')
    if length == L_in:
        return tensor
    O = I = 1
    for n in shape[:axis]:
        O *= n
    for n in shape[axis + 1:]:
        I *= n
    out_shape = shape[:axis] + (length,) + shape[axis + 1:]
    return _PadFunction.apply(tensor.contiguous(), O, L_in, length, I, _fill_bits(constant_values, tensor.dtype), out_shape)


class FixLengthLayer(Layer):
    """Cut or fill the axis `axis` of the input to `length` (pad_or_truncate as a layer)."""

    def __init__(self, length, axis, constant_values=0, **kwargs):
        """
        Args:
            length (int): the length of the axis afterwards.
            axis (int): the axis to cut or fill.
            constant_values (optional): the value that fills. Defaults to 0.
        """
        super().__init__(**kwargs)
        self.length = length
        self.axis = axis
        self.constant_values = constant_values

    def call(self, inputs):
        return pad_or_truncate(inputs, self.length, self.axis, self.constant_values)
