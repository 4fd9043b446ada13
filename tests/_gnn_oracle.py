"""fp64 torch oracle of SparseGNNLayer: the reference's dense formulation (rec_now/layers/sparse_gnn_layer.py:227-236) -- transpose to
(B, D, F), scatter the weight vector into an (F, F) matrix at the sorted [neighbor_idx, field_idx] list, matmul, add, activation.
Autograd on it gives dx and every weight gradient."""
import torch

ACTS = {None: lambda t: t, 'linear': lambda t: t, 'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}


def sorted_indices(fields, field2neighbors):
    """The reference's _generate_indices: ascending [neighbor_idx, field_idx] pairs."""
    idx = {f: i for i, f in enumerate(fields)}
    return sorted([idx[n], i] for i, f in enumerate(fields) for n in field2neighbors.get(f, []))


def dense_weights(indices, w, num_fields):
    """tf.sparse.to_dense(SparseTensor(indices, w, (F, F)))."""
    W = torch.zeros(num_fields, num_fields, dtype=w.dtype)
    if len(indices) == 0:
        return W
    ix = torch.as_tensor(indices, dtype=torch.long)
    return W.index_put((ix[:, 0], ix[:, 1]), w)


def sparse_gnn(x_bdf, indices, weights, num_layers, activation='tanh'):
    """x_bdf (B, D, F) fp64; weights: list of n_sets (E,) tensors, layer i uses weights[i % n_sets]; activation: a name or a callable.
    Returns the list of every layer's (B, D, F) output."""
    act = ACTS[activation] if activation is None or isinstance(activation, str) else activation
    F = x_bdf.shape[-1]
    outs, o = [], x_bdf
    for i in range(num_layers):
        o = act(o + torch.matmul(o, dense_weights(indices, weights[i % len(weights)], F)))
        outs.append(o)
    return outs


def sparse_gnn_bfd(x_bfd, indices, weights, num_layers, activation='tanh'):
    """The same from a (B, F, D) input, with the reference's physical transpose."""
    return sparse_gnn(x_bfd.transpose(1, 2), indices, weights, num_layers, activation)
