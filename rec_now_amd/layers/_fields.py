"""The field inputs of the per-sample interaction layers (AFMLayer, InteractingLayer, BilinearInteractionLayer): a (B, F, D) tensor or a list of
F equal (B, D) tensors, and the device pointer tables their kernels take."""
import torch

from .. import _lib


def check_fields(layer_name, shapes, allow_3d=True):
    """(F, D) of a list of F equal (B, D) shapes or, with allow_3d, of a (B, F, D) shape."""
    takes = 'a (B, F, D) tensor or a list of (B, D) field tensors' if allow_3d else 'a list of (B, D) field tensors'
    is_list = isinstance(shapes, (list, tuple)) and len(shapes) > 0 and isinstance(shapes[0], (list, tuple, torch.Size))
    if is_list:
        first = tuple(shapes[0])
        if len(first) != 2:
            raise ValueError('%s fields must be (B, D) tensors, got shape %s' % (layer_name, first))
        for s in shapes:
            if tuple(s) != first:
                raise ValueError('all %s fields must have the same (B, D) shape, got %s and %s' % (layer_name, first, tuple(s)))
        return len(shapes), int(first[1])
    if not allow_3d:
        raise ValueError('%s takes %s' % (layer_name, takes))
    shape = tuple(shapes) if isinstance(shapes, (list, tuple, torch.Size)) else ()
    if len(shape) != 3:
        raise ValueError('%s takes %s, got shape %s' % (layer_name, takes, shape))
    return int(shape[1]), int(shape[2])


def field_table(xs, what):
    """(tensors kept alive, pointer table, row stride) of F (B, D) fields that share one row stride and have unit column stride --
    views of one (B, F, D) or (B, F*D) tensor pass as they are; anything else is made contiguous."""
    B, D = xs[0].shape
    stride = xs[0].stride(0) if B > 1 else D
    if not all(x.dtype == torch.float32 and (D == 1 or x.stride(1) == 1) and (B <= 1 or x.stride(0) == stride) for x in xs) or stride < D:
        xs = [_lib.f32c(x, what) for x in xs]
        stride = D
    return xs, _lib.ptr_array(xs, xs[0].device), stride


def rows_table(x):
    """Pointer table of the F column blocks x[:, f] of a contiguous float32 (B, F, D) tensor (their common row stride is F * D)."""
    _, F, D = x.shape
    return _lib.const_array([x.data_ptr() + 4 * f * D for f in range(F)], torch.int64, x.device)
