"""fp64 oracle of StarDenseLayer / StackedDenseLayer and their parasitic forms: the reference's own (B, D, U) formulation
(reference rec_now/layers/star_dense_layer.py:118-163, :251-311; stacked_dense_layer.py:116-155, :185-205) restated in torch.
Autograd through it gives the gradients the HIP kernels are compared against."""
import dense_ref as R


def _split(params, B, D, U):
    return [p[:, :D * U].reshape(B, D, U) for p in params], [p[:, D * U:].reshape(B, 1, U) for p in params]


def star_dense(x, kernel, bias, params, activation=None):
    """Weff = kernel * prod P_k[:DU]; beff = sum P_k[DU:] + bias - K."""
    B, D = x.shape
    U = kernel.shape[1]
    ks, bs = _split(params, B, D, U)
    kf = kernel.unsqueeze(0)
    for k in ks:
        kf = kf * k
    bf = sum(bs[1:], bs[0])
    if bias is not None:
        bf = bf + bias
    bf = bf - len(params)
    return _finish(x, kf, bf, activation)


def stacked_dense(x, kernel, bias, params, resnet_weight=1.0, activation=None):
    """Weff = kernel + w sum P_k[:DU]; beff = bias + w sum P_k[DU:]."""
    B, D = x.shape
    U = kernel.shape[1]
    ks, bs = _split(params, B, D, U)
    kf, bf = sum(ks[1:], ks[0]), sum(bs[1:], bs[0])
    if resnet_weight != 1.0:
        kf, bf = resnet_weight * kf, resnet_weight * bf
    kf = kf + kernel.unsqueeze(0)
    if bias is not None:
        bf = bf + bias
    return _finish(x, kf, bf, activation)


def _finish(x, kf, bf, activation):
    return R._act(activation)((x.unsqueeze(1) @ kf + bf).squeeze(1))


def parasitic_dense(x, trunk_kernel, trunk_bias, parasitic_kernel, parasitic_bias, group_idx, mode, activation=None):
    """mode 'star': kernel = trunk * pk[g]; 'stacked': trunk + pk[g]; bias = trunk_bias + pb[g]; group_idx None: trunk alone."""
    k, b = trunk_kernel, trunk_bias
    if group_idx is not None:
        k = k * parasitic_kernel[group_idx] if mode == 'star' else k + parasitic_kernel[group_idx]
        if b is not None:
            b = b + parasitic_bias[group_idx]
    out = x @ k
    if b is not None:
        out = out + b
    return R._act(activation)(out)
