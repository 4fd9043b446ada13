"""fp64 oracle of CANLayer: the reference's own formulation (reference rec_now/layers/can_layer.py:228-275) restated in torch on the
CPU -- the parameter row cut into per-layer kernels viewed as (B, 1, din, dout), one broadcast matmul per layer against the
(B, L, 1, din) input, the all-zero mask, the combiner.  Autograd through it gives the gradients the HIP kernels are compared against;
torch.amax / amin share the gradient equally among ties, as TensorFlow's reduce_max / reduce_min do."""
import torch

import dense_ref as R


def param_size(input_dim, dims, use_bias=True):
    total, din = 0, input_dim
    for dout in dims:
        total += din * dout + (dout if use_bias else 0)
        din = dout
    return total


def can_layer(inputs, dnn_params, dims, activation='tanh', use_bias=True, use_res_net=False, output_layer_use_activation=False,
              output_combiner='sum', mask_all_zero_embedding=True):
    """inputs (B, L, D0) or (B, D0), dnn_params (B, P) -> (B, Dn), or (B, L, Dn) with output_combiner None."""
    act = R._act(activation)
    two_d = inputs.dim() == 2
    x = inputs.unsqueeze(1) if two_d else inputs
    B, L, din = x.shape
    h = x.unsqueeze(2)                                           # (B, L, 1, D0)
    at = 0
    for k, dout in enumerate(dims):
        kernel = dnn_params[:, at:at + din * dout].reshape(B, 1, din, dout)
        at += din * dout
        o = torch.matmul(h, kernel)                              # (B, L, 1, dout)
        if use_bias:
            o = o + dnn_params[:, at:at + dout].reshape(B, 1, 1, dout)
            at += dout
        if output_layer_use_activation or k != len(dims) - 1:
            o = act(o)
        if use_res_net:
            o = h + o
        h, din = o, dout
    assert at == dnn_params.shape[1]
    if mask_all_zero_embedding:
        h = h * (x != 0).any(dim=-1, keepdim=True).unsqueeze(-1).to(h.dtype)
    out = h.squeeze(2)                                           # (B, L, Dn)
    if two_d:
        return out.squeeze(1)
    if output_combiner is None:
        return out
    if callable(output_combiner):
        return output_combiner(out)
    return {'sum': lambda v: v.sum(1), 'mean': lambda v: v.mean(1), 'max': lambda v: torch.amax(v, 1),
            'min': lambda v: torch.amin(v, 1)}[output_combiner](out)
