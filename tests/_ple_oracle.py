"""The fp64 oracle of a built PLELayer / MMOELayer: the `layers` structure that oracle/dense_ref.ple_layer wants, read off the layer's own modules
(layer.dnns[l][g] is the _ExpertDNN stack of group g at PLE layer l, layer.gates[l][g] its _GateDense or None), with the map from every oracle
tensor back to its key in named_weights() -- so that EVERY weight gradient of the layer can be compared with the oracle's."""
import numpy as np
import torch


def _leaf(p):
    return p.detach().cpu().double().requires_grad_(True)


def oracle_layers(layer, to=_leaf):
    """(layers, by_key): layers = list over PLE layers of {'dnn': per group [(kernel (N, Din, U), bias (N, 1, U) | None) per Dense], 'gate': per
    group (kernel (Din, units), bias (units,)) | None}; by_key = {named_weights() key: the oracle tensor made from it}."""
    names = {id(p): k for k, p in layer.named_weights().items()}
    by_key = {}

    def conv(p):
        if p is None:
            return None
        t = to(p)
        by_key[names[id(p)]] = t
        return t

    layers = []
    for stacks, gates in zip(layer.dnns, layer.gates):
        layers.append({'dnn': [[(conv(d.kernel), conv(d.bias)) for d in stack.layers_] for stack in stacks],
                       'gate': [None if g is None else (conv(g.kernel), conv(g.bias)) for g in gates]})
    assert set(by_key) == set(names.values()), 'the oracle structure misses weights: %r' % sorted(set(names.values()) - set(by_key))
    return layers, by_key


def mmoe_oracle_weights(layer, to=_leaf):
    """(expert_kernels, expert_biases, gate_kernel, gate_bias, by_key) of a built MMOELayer, for oracle/dense_ref.mmoe_layer"""
    names = {id(p): k for k, p in layer.named_weights().items()}
    by_key = {}

    def conv(p):
        t = to(p)
        by_key[names[id(p)]] = t
        return t

    ks, bs = [conv(d.kernel) for d in layer.dnn_experts], [conv(d.bias) for d in layer.dnn_experts]
    gk, gb = conv(layer.gates.kernel), conv(layer.gates.bias)
    assert set(by_key) == set(names.values())
    return ks, bs, gk, gb, by_key


def scaled_rows(rng, B, D, sigma=1.0):
    """(B, D) normal inputs, row b scaled by 2^-(b % 9)"""
    return (rng.normal(0, sigma, (B, D)) * np.exp2(-(np.arange(B) % 9).astype(np.float64))[:, None]).astype(np.float32)


def row_margin(ref, got, rel):
    """worst |err| / (rel max |ref| of the row) over the rows of a (.., B, W) tensor"""
    ref = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(got, np.float64) - ref).max(-1)
    return float((err / np.maximum(rel * np.abs(ref).max(-1), 1e-300)).max())


def column_margin(ref, got, rel):
    """worst |err| / (rel max |ref| of the column): kernels (N, Din, U) and biases (N, 1, U) per expert slice n and column u, a gate kernel
    (Din, units) per column, a gate bias (units,) per entry"""
    ref = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(got, np.float64) - ref)
    if ref.ndim >= 2:
        ax = ref.ndim - 2
        err, ref = err.max(ax), np.abs(ref).max(ax)
    return float((err / np.maximum(rel * np.abs(ref), 1e-300)).max())


def torch_np(t):
    return t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)
