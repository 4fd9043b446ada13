"""Turn one weight per embedding into one weight per element of the concatenated embeddings -- drop-in for
rec_now/rec_block/embedding_wise_weight.py.

The input of a DNN is usually (batch_size, sum(embedding_dim)) with embeddings of different widths; a weight computed per embedding has to be spread
to that shape before it can scale the input.  gather_embedding_element_wise_weight does that; apply_embedding_element_wise_weight multiplies the
input with the spread weights in the same kernel, so the (batch_size, sum(embedding_dim)) weight tensor is never written.

Host side of k_elw_fwd / k_elw_bwd of csrc/tensor_util.hip.  The gradient to the weights goes through the inverse of pos_idx as a CSR table (one
thread owns one (row, embedding) and adds its positions in ascending order): no atomics, bit-identical from run to run.
"""
import numpy as np
import torch

from .. import _lib


def _csr_inverse(pos, num_embedding):
    """Inverse of the position table: (off, idx) with idx[off[e]:off[e + 1]] = the positions p of embedding e (pos[p] == e) in ascending order."""
    pos = np.asarray(pos, dtype=np.int64).reshape(-1)
    idx = np.argsort(pos, kind='stable')
    off = np.zeros(num_embedding + 1, dtype=np.int64)
    np.cumsum(np.bincount(pos, minlength=num_embedding), out=off[1:])
    return [int(v) for v in off], [int(v) for v in idx]


_CSR = {}


def _csr_device(pos, num_embedding, device):
    """The CSR inverse of `pos` as two int32 device arrays: built once per table, uploaded once per content (_lib.const_array)."""
    key = (num_embedding, pos)
    hit = _CSR.get(key)
    if hit is None:
        if len(_CSR) >= 256:
            _CSR.clear()
        off, idx = _csr_inverse(pos, num_embedding)
        hit = _CSR[key] = (tuple(off), tuple(idx))
    return _lib.const_array(hit[0], torch.int32, device), _lib.const_array(hit[1], torch.int32, device)


def _position_table(pos_idx, num_embedding):
    """pos_idx (list, tuple, numpy array or tensor of shape (P,) or (1, P)) -> tuple of P ints, checked against [0, num_embedding)."""
    if isinstance(pos_idx, torch.Tensor):
        pos_idx = pos_idx.detach().cpu().numpy()            # the one host read of a tensor-valued table
    arr = np.asarray(pos_idx)
    if arr.size and not np.issubdtype(arr.dtype, np.integer):
        raise TypeError('pos_idx must hold integers, got %s' % arr.dtype)
    if arr.ndim == 2 and arr.shape[0] == 1:
        arr = arr[0]
    elif arr.ndim == 2:
        raise NotImplementedError('a per-sample position table of shape %s is not supported: pos_idx must be (P,) or (1, P)' % (tuple(arr.shape),))
    if arr.ndim != 1:
        raise ValueError('pos_idx must have the shape (P,) or (1, P), got %s' % (tuple(arr.shape),))
    if arr.size and (int(arr.min()) < 0 or int(arr.max()) >= num_embedding):
        raise ValueError('pos_idx entries must lie in [0, %d), got %d .. %d' % (num_embedding, int(arr.min()), int(arr.max())))
    return tuple(int(v) for v in arr)


class _ElemWeightFunction(torch.autograd.Function):
    """out (B, P) = w[:, pos] (x is None) or x * w[:, pos]."""

    @staticmethod
    def forward(ctx, w, x, pos):
        B, E = w.shape
        P = len(pos)
        dev = w.device
        pos_d = _lib.const_array(pos, torch.int32, dev)
        out = torch.empty((B, P), dtype=torch.float32, device=dev)                     # every element is written by the kernel
        _lib.call('recnow_elem_weight_fwd', _lib.ptr(w), _lib.ptr(pos_d), _lib.ptr(x), B, E, P, _lib.ptr(out), _lib.stream())
        need_dw, need_dx = ctx.needs_input_grad[0], x is not None and ctx.needs_input_grad[1]
        ctx.save_for_backward(x if need_dw else None, w if need_dx else None)
        ctx.meta = (B, E, P, pos, need_dw, need_dx, x is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        B, E, P, pos, need_dw, need_dx, fused = ctx.meta
        if not (need_dw or need_dx):
            return None, None, None
        g = _lib.f32c(g, 'grad')
        dev = g.device
        off = idx = None
        if need_dw:
            off, idx = _csr_device(pos, E, dev)
        dw = torch.empty((B, E), dtype=torch.float32, device=dev) if need_dw else None
        dx = torch.empty((B, P), dtype=torch.float32, device=dev) if need_dx else None
        _lib.call('recnow_elem_weight_bwd', _lib.ptr(g), _lib.ptr(x), _lib.ptr(w), _lib.ptr(_lib.const_array(pos, torch.int32, dev)), _lib.ptr(off),
                  _lib.ptr(idx), B, E, P, _lib.ptr(dw), _lib.ptr(dx), _lib.stream())
        return dw, dx, None


def _weights_2d(embedding_weights):
    if not isinstance(embedding_weights, torch.Tensor):
        raise TypeError('embedding_weights must be a torch.Tensor, got %s' % type(embedding_weights))
    if embedding_weights.dim() != 2:
        raise ValueError('embedding_weights must be (batch_size, num_embedding), got a tensor of rank %d' % embedding_weights.dim())
    return embedding_weights


def gather_embedding_element_wise_weight(embedding_weights, pos_idx):
    """Spread the weight of each embedding to the elements of that embedding.

    Args:
        embedding_weights: (batch_size, num_embedding) float32 GPU tensor, the weight of each embedding.
        pos_idx: sum(embedding_dim) integers in [0, num_embedding): the embedding each position of the DNN input belongs to.  A list, tuple or
            numpy array keeps the call free of host synchronisation (the table is uploaded once per content and cached); a tensor -- of shape
            (P,) or (1, P) -- is read back to the host on every call, which synchronises.  Entries outside [0, num_embedding) raise
            ValueError; a per-sample (batch_size, P) table raises NotImplementedError.

    Returns:
        (batch_size, sum(embedding_dim)) float32: out[b][p] = embedding_weights[b][pos_idx[p]].
    """
    w = _weights_2d(embedding_weights)
    pos = _position_table(pos_idx, w.shape[1])
    return _ElemWeightFunction.apply(_lib.f32c(w, 'embedding_weights'), None, pos)


def apply_embedding_element_wise_weight(inputs, embedding_weights, pos_idx):
    """inputs * gather_embedding_element_wise_weight(embedding_weights, pos_idx) in one kernel: the element-wise weight tensor is never written.

    Args:
        inputs: (batch_size, sum(embedding_dim)) float32 GPU tensor, the concatenated embeddings.
        embedding_weights, pos_idx: as gather_embedding_element_wise_weight.

    Returns:
        (batch_size, sum(embedding_dim)) float32: out[b][p] = inputs[b][p] * embedding_weights[b][pos_idx[p]]; gradients reach both tensors.
    """
    w = _weights_2d(embedding_weights)
    pos = _position_table(pos_idx, w.shape[1])
    if not isinstance(inputs, torch.Tensor):
        raise TypeError('inputs must be a torch.Tensor, got %s' % type(inputs))
    if tuple(inputs.shape) != (w.shape[0], len(pos)):
        raise ValueError('inputs must be (batch_size, len(pos_idx)) = %s, got %s' % ((w.shape[0], len(pos)), tuple(inputs.shape)))
    return _ElemWeightFunction.apply(_lib.f32c(w, 'embedding_weights'), _lib.f32c(inputs, 'inputs'), pos)
