"""CANLayer -- drop-in for rec_now/layers/can_layer.py (co-action network, arXiv 2011.05625): every sample transforms its L input
embeddings with a small MLP whose kernels and biases are that sample's row of a second input, `dnn_params`.

The reference reshapes each parameter row to a (B, 1, din, dout) kernel, runs one broadcast batched matmul per layer and keeps a
(B, L, 1, D_k) activation per layer for autograd.  Here one HIP kernel per direction (csrc/can.hip) gives one workgroup to a sample:
the sample's parameters are read once into LDS, the layer chain, the all-zero mask and the combiner run on-chip, and the backward
recomputes the chain, so the layer allocates its output and its two gradients and nothing else.

Symbols: B batch size, L embeddings per sample (an all-zero embedding is padding), D0 the embedding width, D1 .. Dn the layer widths,
P = sum_k D_{k-1} D_k [+ D_k] the width of a parameter row: per layer the kernel, row-major (din, dout), then the bias.
"""
import ctypes
import math

import torch

from .. import _lib
from ._keras import ACT_RELU, ACT_SIGMOID, ACT_TANH, Layer, activation_code

_COMBINERS = {None: -1, 'sum': 0, 'mean': 1, 'max': 2, 'min': 3}          # -1 or RECNOW_REDUCE_* of include/recnow.h
_CALLABLE_ACTS = {torch.tanh: ACT_TANH, torch.relu: ACT_RELU, torch.sigmoid: ACT_SIGMOID}
_MAX_DIM, _MAX_LAYERS = 64, 8                                              # CAN_MAX_DIM, CAN_MAX_LAYERS of csrc/can.hip


def _c_dims(dims):
    return (ctypes.c_int * len(dims))(*dims)


def can_supported(input_dim, dnn_dims, use_bias=True):
    """Whether the kernels take this network (host-only query of the library, no device call)."""
    dims = [int(d) for d in dnn_dims]
    return bool(_lib.load().recnow_can_supported(int(input_dim), _c_dims(dims), len(dims), int(bool(use_bias))))


class _CANFunction(torch.autograd.Function):
    """(x (B, L, D0), params (B, P)) -> (B, L, Dn), or (B, Dn) with a combiner.  Saves its two inputs (and y for max / min): the
    backward kernel recomputes every activation."""

    @staticmethod
    def forward(ctx, x, params, dims, act, use_bias, res_net, last_act, mask, comb):
        B, L, D0 = x.shape
        y = torch.empty((B, L, dims[-1]) if comb < 0 else (B, dims[-1]), dtype=torch.float32, device=x.device)
        flags = (act, int(use_bias), int(res_net), int(last_act), int(mask), comb)
        if y.numel() > 0:
            _lib.call('recnow_can_fwd', _lib.ptr(x), _lib.ptr(params), _lib.ptr(y), B, L, D0, _c_dims(dims), len(dims), *flags, _lib.stream())
        if comb >= _COMBINERS['max']:
            ctx.save_for_backward(x, params, y)
        else:
            ctx.save_for_backward(x, params)
        ctx.meta = (dims, flags)
        return y

    @staticmethod
    def backward(ctx, g):
        dims, flags = ctx.meta
        x, params = ctx.saved_tensors[:2]
        y = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        B, L, D0 = x.shape
        need_x, need_p = ctx.needs_input_grad[:2]
        g = _lib.f32c(g, 'grad')
        dx = torch.empty_like(x) if need_x else None                    # every element is written by the kernel
        dp = torch.empty_like(params) if need_p else None
        if B > 0 and (need_x or need_p):
            _lib.call('recnow_can_bwd', _lib.ptr(x), _lib.ptr(params), _lib.ptr(g), _lib.ptr(y), B, L, D0, _c_dims(dims), len(dims), *flags,
                      _lib.ptr(dx), _lib.ptr(dp), _lib.stream())
        return dx, dp, None, None, None, None, None, None, None


class CANLayer(Layer):
    """co-action network: `inputs` transformed by the per-sample DNN whose parameters are `dnn_params`."""
    CAN_EXPANDED_INPUT_DIM = 4      # the rank the reference expands its input to; kept for callers that read it

    def __init__(self, dnn_dims=None, activation='tanh', use_bias=True, use_res_net=False, output_layer_use_activation=False,
                 output_combiner='sum', mask_all_zero_embedding=True, **kwargs):
        """
        Args:
            dnn_dims: the layer widths D1 .. Dn; None: as many layers of width D0 as the parameter row holds.
            activation: None / 'linear', 'relu', 'tanh', 'sigmoid', or torch.tanh / torch.relu / torch.sigmoid.  The activation runs
                inside the kernel, between the layers, so no other callable can be applied: NotImplementedError.
            use_bias: every layer's kernel is followed by a bias in the parameter row.
            use_res_net: h_k = h_{k-1} + act(...); every width must then equal D0.
            output_layer_use_activation: apply the activation on the last layer too.
            output_combiner: None, 'sum', 'mean', 'max', 'min' or a callable on the (B, L, Dn) result; unused for a (B, D0) input.
            mask_all_zero_embedding: the output of an all-zero embedding (padding) is zero.
        """
        super().__init__(**kwargs)
        self.dnn_dims = dnn_dims
        self.use_bias = use_bias
        self.activation = activation
        if callable(activation):
            if activation not in _CALLABLE_ACTS:
                raise NotImplementedError('CANLayer applies its activation inside the fused kernel: linear (None), relu, tanh or sigmoid '
                                          '(by name, or torch.relu / torch.tanh / torch.sigmoid); got %r' % (activation,))
            self.act_code = _CALLABLE_ACTS[activation]
        else:
            self.act_code = activation_code(activation)[0]
        self.use_res_net = use_res_net
        self.output_layer_use_activation = output_layer_use_activation
        if not callable(output_combiner) and output_combiner not in _COMBINERS:
            raise ValueError("combiner must be one of None, 'mean', 'sum', 'max', 'min' or a callable object")
        self.output_combiner = output_combiner
        self.mask_all_zero_embedding = mask_all_zero_embedding

    @classmethod
    def _get_layer_param_size(cls, dim_in, dim_out, use_bias):
        """Parameters of one layer: the kernel and, with use_bias, the bias."""
        return dim_in * dim_out + (dim_out if use_bias else 0)

    @classmethod
    def get_dnn_param_size(cls, input_dim, dnn_dims, use_bias=True):
        """Parameters of the whole DNN = the width P of a row of `dnn_params`."""
        total, dim_in = 0, input_dim
        for dim_out in dnn_dims:
            total += cls._get_layer_param_size(dim_in, dim_out, use_bias)
            dim_in = dim_out
        return total

    @classmethod
    def _has_non_zero(cls, tensor, axis=-1, keepdims=True):
        """bool: whether `tensor` has a non-zero element along `axis` (-0.0 is zero)."""
        return (tensor != 0).any(dim=axis, keepdim=keepdims)

    def _auto_decide_dnn_param_size(self, input_dim, total_param_size):
        """The widths of a DNN whose layers all have the input's width: total_param_size must hold a whole number of them."""
        one_layer_param_size = self._get_layer_param_size(input_dim, input_dim, self.use_bias)
        n_layer = float(total_param_size) / one_layer_param_size
        if math.floor(n_layer) != n_layer:
            raise ValueError('dnn_param_size not match! input_dim: %d, total_param_size: %d, use_bias:%s, one_layer_param_size(auto decide): %d'
                             % (input_dim, total_param_size, self.use_bias, one_layer_param_size))
        return [input_dim] * int(n_layer)

    def _check_dnn_param_size(self, input_dim, dnn_dims, size_dnn_param):
        """The parameter row must be exactly as wide as `dnn_dims` needs."""
        expected = self.get_dnn_param_size(input_dim, dnn_dims, self.use_bias)
        if expected != size_dnn_param:
            raise ValueError('dnn_param_size not match! input_dim: %d, expected total_param_size: %d,\nuse_bias:%s, dnn_dims: %s, '
                             'calculated total_param_size: %d' % (input_dim, size_dnn_param, self.use_bias, str(dnn_dims), expected))

    def _get_dnn_dims(self, dim_in, size_dnn_param):
        if self.dnn_dims is None:
            return self._auto_decide_dnn_param_size(dim_in, size_dnn_param)
        return [int(d) for d in self.dnn_dims]

    def call(self, inputs, dnn_params):
        """inputs (B, L, D0) or (B, D0), dnn_params (B, P): float32 GPU tensors.  Returns (B, Dn) with a combiner or for a (B, D0) input,
        (B, L, Dn) with output_combiner=None."""
        for t, what in ((inputs, 'inputs'), (dnn_params, 'dnn_params')):
            if not isinstance(t, torch.Tensor):
                raise TypeError('%s must be a torch.Tensor, got %s' % (what, type(t)))
            if t.dtype != torch.float32:
                raise TypeError('CANLayer computes in float32; %s is %s' % (what, t.dtype))
        if inputs.dim() not in (2, 3):
            raise ValueError('inputs must be (B, L, D0) or (B, D0), got shape %s' % (tuple(inputs.shape),))
        if dnn_params.dim() != 2 or dnn_params.shape[0] != inputs.shape[0]:
            raise ValueError('dnn_params must be (B, size_dnn_param) with B = %d, got shape %s' % (inputs.shape[0], tuple(dnn_params.shape)))
        dim_in, size_dnn_param = int(inputs.shape[-1]), int(dnn_params.shape[-1])
        dnn_dims = self._get_dnn_dims(dim_in, size_dnn_param)
        self._check_dnn_param_size(dim_in, dnn_dims, size_dnn_param)
        if self.use_res_net and any(d != dim_in for d in dnn_dims):
            raise ValueError('use_res_net adds each layer\'s input to its output: every entry of dnn_dims must equal the input dim %d, got %s'
                             % (dim_in, dnn_dims))
        if not dnn_dims or not can_supported(dim_in, dnn_dims, self.use_bias):
            raise NotImplementedError('CANLayer kernels take an input dim and layer dims of 1..%d, 1..%d layers, and a parameter row that fits, '
                                      'with the backward\'s staging, the 64 KB of LDS of one workgroup; got input dim %d, dnn_dims %s '
                                      '(%d parameters)' % (_MAX_DIM, _MAX_LAYERS, dim_in, dnn_dims, size_dnn_param))
        combiner = self.output_combiner
        is_2d = inputs.dim() == 2
        fused = -1 if is_2d or callable(combiner) else _COMBINERS[combiner]
        x = inputs.unsqueeze(1) if is_2d else inputs
        if fused >= 0 and x.shape[1] == 0:
            raise ValueError("cannot reduce over an empty axis (shape %s, axis 1) with '%s'" % (tuple(x.shape[:2]) + (dnn_dims[-1],), combiner))
        _lib.require_gpu(inputs, 'inputs')                  # after the argument checks: those hold on any device
        _lib.require_gpu(dnn_params, 'dnn_params')
        out = _CANFunction.apply(x.contiguous(), dnn_params.contiguous(), tuple(dnn_dims), self.act_code, self.use_bias, self.use_res_net,
                                 self.output_layer_use_activation, self.mask_all_zero_embedding, fused)
        if is_2d:
            return out.squeeze(1)
        if callable(combiner):
            return combiner(out)
        return out
