"""numpy fp64 restatement, from their definitions, of the three tensor ops of csrc/tensor_util.hip and of their gradients:
reduce over an axis (PoolingLayer), pad or truncate an axis (FixLengthLayer), element-wise embedding weights.  Shared by the CPU and GPU tests."""
import numpy as np


def _axes(ndim, axis):
    if axis is None:
        return tuple(range(ndim))
    if isinstance(axis, (list, tuple)):
        return tuple(sorted(a % ndim for a in axis))
    return (axis % ndim,)


def reduce_axis(x, axis, keepdims, combiner):
    """sum / mean / max / min of x over `axis` (int, None or a sequence), computed in fp64."""
    x = np.asarray(x, dtype=np.float64)
    fn = {'sum': np.sum, 'mean': np.mean, 'max': np.max, 'min': np.min}[combiner]
    return fn(x, axis=_axes(x.ndim, axis), keepdims=keepdims)


def reduce_axis_grad(x, axis, keepdims, combiner, g):
    """d <g, reduce(x)> / d x.  sum: g broadcast; mean: g / n; max / min: g / count at every position that equals the result, count = the number
    of such positions among the reduced ones (TensorFlow's rule: ties share the gradient equally)."""
    x = np.asarray(x, dtype=np.float64)
    axes = _axes(x.ndim, axis)
    g = np.asarray(g, dtype=np.float64)
    if not keepdims:
        g = np.expand_dims(g, axes) if axes else g
    n = 1
    for a in axes:
        n *= x.shape[a]
    if combiner == 'sum':
        return np.broadcast_to(g, x.shape).copy()
    if combiner == 'mean':
        return np.broadcast_to(g / n, x.shape).copy()
    y = (np.max if combiner == 'max' else np.min)(x, axis=axes, keepdims=True)
    hit = x == y
    count = hit.sum(axis=axes, keepdims=True)
    return np.where(hit, g / count, 0.0)


def pad_or_truncate(x, length, axis=-1, constant_values=0):
    """x with shape[axis] cut to `length`, or filled up at the end of that axis with constant_values.  The dtype is kept."""
    x = np.asarray(x)
    axis = axis % x.ndim
    shape = list(x.shape)
    shape[axis] = length
    out = np.full(shape, constant_values, dtype=x.dtype)
    keep = min(length, x.shape[axis])
    sel = tuple(slice(0, keep) if d == axis else slice(None) for d in range(x.ndim))
    out[sel] = x[sel]
    return out


def pad_or_truncate_grad(in_shape, length, axis, g):
    """d <g, pad_or_truncate(x)> / d x: g over the kept part, zero over the part that was cut off."""
    return pad_or_truncate(np.asarray(g), in_shape[axis % len(in_shape)], axis, 0)


def csr_inverse(pos, num_embedding):
    """(off, idx): idx[off[e]:off[e + 1]] lists, in ascending order, the positions p with pos[p] == e."""
    lists = [[] for _ in range(num_embedding)]
    for p, e in enumerate(pos):
        lists[e].append(p)
    off = [0]
    for l in lists:
        off.append(off[-1] + len(l))
    return off, [p for l in lists for p in l]


def gather_weight(w, pos):
    """out[b][p] = w[b][pos[p]] (the dtype of w is kept: a copy)."""
    return np.asarray(w)[:, np.asarray(pos, dtype=np.int64)]


def apply_weight(x, w, pos):
    return np.asarray(x, dtype=np.float64) * gather_weight(np.asarray(w, dtype=np.float64), pos)


def elem_weight_grads(x, w, pos, g):
    """(dw, dx) of <g, x * w[:, pos]>; x = None: the gather alone (dx is None)."""
    g = np.asarray(g, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    gx = g if x is None else g * np.asarray(x, dtype=np.float64)
    dw = np.zeros_like(w)
    for p, e in enumerate(pos):
        dw[:, e] += gx[:, p]
    return dw, (None if x is None else g * gather_weight(w, pos))
