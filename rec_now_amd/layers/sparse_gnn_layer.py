"""SparseGNNLayer -- drop-in for rec_now/layers/sparse_gnn_layer.py: graph convolution over the field embeddings of a row.

The fields are the nodes of a hand-given directed graph; every layer replaces a node by act(node + weighted sum of its neighbours),
with one trainable weight per edge.  The reference transposes the input to (B, D, F) and multiplies it by a dense (F, F) matrix per layer;
here one HIP kernel per direction (csrc/sparse_gnn.hip) runs all layers on tiles that stay on chip: the forward reads the input once and
writes each requested output once, the backward recomputes the layer chain from the input instead of keeping the layer outputs.

Two routes, chosen per layer object with `route=`: 'edges' walks the edge list (csrc/sparse_gnn.hip, at most 64 fields, cost per edge), 'dense'
multiplies by the dense matrix I + W on the matrix cores (csrc/sparse_gnn_dense.hip, at most 128 fields, cost independent of the edges), 'auto'
takes the faster one by the measured table below (auto_route).
"""
import logging

import torch

from .. import _lib
from ._keras import Layer, activation_code

DEFAULT_NEIGHBOR_INITIAL_WEIGHT = 0.1
MAX_FIELDS = 64                      # SG_MAXF of csrc/sparse_gnn.hip
MAX_FIELDS_DENSE = 128               # SD_MAXF of csrc/sparse_gnn_dense.hip
ROUTES = ('edges', 'dense', 'auto')
LAYOUT_BFD, LAYOUT_BDF, LAYOUT_LIST = 0, 1, 2      # RECNOW_GNN_* of include/recnow.h


def _default_initializer(shape, generator=None):
    return torch.full(tuple(shape), DEFAULT_NEIGHBOR_INITIAL_WEIGHT)


def edge_tables(indices, num_fields):
    """The kernel's edge tables from the sorted [source, destination] list (entry k belongs to weight k).
    Returns a dict of int lists: by destination `dptr` (F+1), `dsrc`, `dwid`; by source `sptr` (F+1), `sdst`, `swid`, `ssrc`."""
    F, E = num_fields, len(indices)
    by_dst = sorted(range(E), key=lambda k: (indices[k][1], indices[k][0]))
    by_src = sorted(range(E), key=lambda k: (indices[k][0], indices[k][1]))
    dptr, sptr = [0] * (F + 1), [0] * (F + 1)
    for s, d in indices:
        dptr[d + 1] += 1
        sptr[s + 1] += 1
    for i in range(F):
        dptr[i + 1] += dptr[i]
        sptr[i + 1] += sptr[i]
    return {'dptr': dptr, 'dsrc': [indices[k][0] for k in by_dst], 'dwid': by_dst,
            'sptr': sptr, 'sdst': [indices[k][1] for k in by_src], 'swid': by_src, 'ssrc': [indices[k][0] for k in by_src]}


CHUNK = 4                            # SG_CHUNK of csrc/sparse_gnn.hip


def chunk_stream(ptr, col, wid, num_fields):
    """One CSR table as the kernel's stream of chunks of CHUNK edges of one node, in node order: a node without edges still has one chunk, and a
    short chunk is padded with edges of weight index -1 that point at the node itself.  Returns (S, G): per chunk 8 ints
    [o0, o1, o2, o3, node, flags (1 first chunk of the node | 2 last), 0, 0] and the 4 weight indices."""
    S, G = [], []
    for i in range(num_fields):
        ks = list(range(ptr[i], ptr[i + 1]))
        n = max(1, -(-len(ks) // CHUNK))
        for c in range(n):
            part = ks[c * CHUNK:(c + 1) * CHUNK]
            pad = CHUNK - len(part)
            S += [col[k] for k in part] + [i] * pad + [i, (1 if c == 0 else 0) | (2 if c == n - 1 else 0), 0, 0]
            G += [wid[k] for k in part] + [-1] * pad
    return S, G


def _pack_tables(t, num_fields):
    """The `tab` array of recnow_sparse_gnn_fwd / _bwd (include/recnow.h)."""
    dS, dG = chunk_stream(t['dptr'], t['dsrc'], t['dwid'], num_fields)
    sS, sG = chunk_stream(t['sptr'], t['sdst'], t['swid'], num_fields)
    return [len(dG) // CHUNK, len(sG) // CHUNK, 0, 0] + dS + dG + sS + sG + t['ssrc'] + t['sdst'] + t['swid']


# route='auto': the fewest edges at which the dense route beat the edge route in BOTH directions, per field count up to which the entry holds.
# The dense route's cost depends on F rounded up to 32 and not on E, the edge route's grows with E, so the rule is a number of edges.
# MI355X, B 65 536, D 32, L 3, tanh, unshared weights, ms forward / backward (profiles/gnn_layer_bench.txt):
#   F 32   in-degree   2 (E 64)       4 (E 128)      8 (E 256)      16 (E 512)     31 (E 992)
#          edges       0.577 / 4.78   0.576 / 5.49   0.865 / 8.63   1.447 / 15.2   2.633 / 27.9
#          dense       0.314 / 1.77   0.316 / 1.74   0.320 / 1.72   0.324 / 1.71   0.322 / 1.71
#   F 64   in-degree   8 (E 512)      32 (E 2048)    63 (E 4032)
#          edges       3.862 / 32.6   11.51 / 111    21.71 / 216
#          dense       1.165 / 6.03   1.168 / 6.03   1.167 / 6.08
# The smallest graphs measured already favour the dense route; below them nothing was measured and the edge route stays.
DENSE_MIN_EDGES = ((32, 64), (64, 512))


def auto_route(num_fields, num_edges):
    """The route `route='auto'` takes: 'dense' above 64 fields (the edge route stops there), or when the graph has at least the measured
    cross-over number of edges of its field count; 'edges' otherwise."""
    if num_fields > MAX_FIELDS:
        return 'dense'
    for fields, edges in DENSE_MIN_EDGES:
        if num_fields <= fields:
            return 'dense' if num_edges >= edges else 'edges'
    return 'edges'


class _SparseGNNFunction(torch.autograd.Function):
    """All layers as one node.  Saves the input, the weights and the edge tables only; `n_out` outputs: every layer's (in one block) or the
    last one's."""

    @staticmethod
    def forward(ctx, meta, w, *xs):
        F, E, L, n_sets, act, in_layout, out_layout, all_layers, tab, dense = meta
        xs = [_lib.f32c(x, 'SparseGNNLayer input') for x in xs]
        wc = _lib.f32c(w.detach(), 'weights')
        dev = xs[0].device
        if in_layout == LAYOUT_LIST:
            B, D = xs[0].shape
            x_ptr, xl_ptr = None, _lib.ptr(_lib.ptr_array(xs, dev))
            aligned = int(all(x.data_ptr() % 16 == 0 for x in xs))
        else:
            B = xs[0].shape[0]
            D = xs[0].shape[1] // F if xs[0].dim() == 2 else xs[0].shape[2 if in_layout == LAYOUT_BFD else 1]
            x_ptr, xl_ptr, aligned = _lib.ptr(xs[0]), None, 0
        shape = (B, F, D) if out_layout == LAYOUT_BFD else (B, D, F)
        tabd = _lib.const_array(tab, torch.int32, dev)       # dense: the E sources, then the E destinations of the sorted edge list
        if all_layers:
            y = torch.empty((L,) + shape, dtype=torch.float32, device=dev)
            y_last, y_all = None, _lib.ptr(_lib.block_ptr_array(y, L)) if B else None
            outs = y.unbind(0)
        else:
            y = torch.empty(shape, dtype=torch.float32, device=dev)
            y_last, y_all = _lib.ptr(y), None
            outs = (y,)
        if B and dense:
            ws = _lib.workspace(_lib.load().recnow_sparse_gnn_dense_workspace_bytes(F, E, n_sets, 0), dev)
            _lib.call('recnow_sparse_gnn_dense_fwd', x_ptr, xl_ptr, in_layout, aligned, out_layout, _lib.ptr(tabd), _lib.ptr(tabd[E:]),
                      _lib.ptr(wc), B, F, D, E, L, n_sets, act, y_last, y_all, int(y.data_ptr() % 16 == 0 and (F * D) % 4 == 0), _lib.ptr(ws),
                      ws.numel(), _lib.stream())
        elif B:
            _lib.call('recnow_sparse_gnn_fwd', x_ptr, xl_ptr, in_layout, aligned, out_layout, _lib.ptr(tabd), _lib.ptr(wc), B, F, D, E, L,
                      n_sets, act, y_last, y_all, int(y.data_ptr() % 16 == 0 and (F * D) % 4 == 0), _lib.stream())
        ctx.save_for_backward(wc, tabd, *xs)
        ctx.meta = (B, D) + tuple(meta[:8]) + (dense,)
        return outs

    @staticmethod
    def backward(ctx, *dys):
        wc, tabd, *xs = ctx.saved_tensors
        B, D, F, E, L, n_sets, act, in_layout, out_layout, all_layers, dense = ctx.meta
        dev = wc.device
        need_w, need_x = ctx.needs_input_grad[1] and E > 0, any(ctx.needs_input_grad[2:])
        dw = torch.empty_like(wc) if need_w else None
        dx = None
        if need_x:
            dx = torch.empty((F, B, D) if in_layout == LAYOUT_LIST else xs[0].shape, dtype=torch.float32, device=dev)
        if ctx.needs_input_grad[1] and E == 0:
            dw = torch.zeros_like(wc)
        if need_w or need_x:
            dys = [None if g is None else _lib.f32c(g, 'grad') for g in dys]
            if all_layers:
                dy_last, dy_all = None, _lib.ptr(_lib.const_array([0 if g is None else g.data_ptr() for g in dys], torch.int64, dev))
                al = int(all(g is None or g.data_ptr() % 16 == 0 for g in dys))
            else:
                dy_last, dy_all, al = _lib.ptr(dys[0]), None, 0
            if in_layout == LAYOUT_LIST:
                x_ptr, xl_ptr = None, _lib.ptr(_lib.ptr_array(xs, dev))
                aligned = int(all(x.data_ptr() % 16 == 0 for x in xs))
            else:
                x_ptr, xl_ptr, aligned = _lib.ptr(xs[0]), None, 0
            if dense:
                ws = _lib.workspace(_lib.load().recnow_sparse_gnn_dense_workspace_bytes(F, E, n_sets, int(need_w)), dev)
                _lib.call('recnow_sparse_gnn_dense_bwd', x_ptr, xl_ptr, in_layout, aligned, out_layout, _lib.ptr(tabd), _lib.ptr(tabd[E:]),
                          _lib.ptr(wc), B, F, D, E, L, n_sets, act, dy_last, dy_all, al, _lib.ptr(dx), _lib.ptr(dw) if need_w else None,
                          _lib.ptr(ws), ws.numel(), _lib.stream())
            else:
                ws = _lib.workspace(_lib.load().recnow_sparse_gnn_workspace_bytes(B, F, D, E, n_sets) if need_w else 0, dev)
                _lib.call('recnow_sparse_gnn_bwd', x_ptr, xl_ptr, in_layout, aligned, out_layout, _lib.ptr(tabd), _lib.ptr(wc), B, F, D, E, L,
                          n_sets, act, dy_last, dy_all, al, _lib.ptr(dx), _lib.ptr(dw) if need_w else None, _lib.ptr(ws), ws.numel(),
                          _lib.stream())
        if dx is None:
            dxs = (None,) * len(xs)
        elif in_layout == LAYOUT_LIST:
            dxs = tuple(dx.unbind(0))
        else:
            dxs = (dx,)
        return (None, dw) + dxs


class SparseGNNLayer(Layer):
    """Feature-interaction layer that convolves over a hand-given graph of the fields.

    Every field is a node; `field2neighbors` lists, per node, the nodes it aggregates (directed edges).  All layers share the graph and,
    unless `share_weights_between_layers`, train their own edge weights.

    Symbols: B batch size, D embedding dim, F number of fields, E number of edges.

    Weights: `weights_{idx}` of shape (E,), one per weight set.  Entry k belongs to the k-th pair of the ascending-sorted list of
    [neighbor_idx, field_idx] (the reference's `_generate_indices`), so reference checkpoints load 1:1.

    A callable activation is applied by torch, layer by layer, around one-layer linear kernel calls.

    route (keyword only): 'edges' (the default) walks the edge list, at most 64 fields; 'dense' multiplies by the dense (F, F) matrix on the
    matrix cores, at most 128 fields, faster on all but the sparsest graphs; 'auto' picks by `auto_route`.  The routes agree to fp32 rounding,
    not bit for bit; weights, checkpoints and state_dict names are the same.
    """

    def __init__(self, fields, field2neighbors, weights_initializer=_default_initializer, num_layers=1,
                 share_weights_between_layers=True, activation='tanh', *, route='edges', **kwargs):
        """fields: list of F hashable field ids; field2neighbors: dict field -> list / set of neighbours, or a list / set of
        (node_to, node_from) pairs; weights_initializer: defaults to the constant 0.1; num_layers; share_weights_between_layers;
        activation: 'linear' / 'relu' / 'tanh' / 'sigmoid' / None, or a callable on torch tensors."""
        super().__init__(**kwargs)
        if route not in ROUTES:
            raise ValueError('route must be one of %s, got %r' % (', '.join(repr(r) for r in ROUTES), route))
        self.route = route
        self.fields = fields
        self.field2neighbors = self._normalize_neighbors(field2neighbors)
        self.field2idx = {field: idx for idx, field in enumerate(fields)}
        self.weights_initializer = weights_initializer
        self.num_layers = int(num_layers)
        if self.num_layers < 1:
            raise ValueError('num_layers must be at least 1, got %s' % num_layers)
        self.share_weights_between_layers = share_weights_between_layers
        self.activation = activation
        self.act_code, self.act_callable = activation_code(activation)
        self._check_fields()
        self._check_field2neighbors()

    def _normalize_neighbors(self, field2neighbors):
        if isinstance(field2neighbors, (list, set)):
            return SparseGNNLayer.list_of_edge_to_neighbors(field2neighbors)
        if not isinstance(field2neighbors, dict):
            raise TypeError('field2neighbors must be one of `list of pairs`, `set of pairs`, '
                            f'`dict of neighbors`, but get {type(field2neighbors)}')
        return field2neighbors

    def _check_fields(self):
        set_fields = set(self.fields)
        if len(set_fields) != len(self.fields):
            raise ValueError(f'{len(self.fields) - len(set_fields)} duplicated fields in fields.')

    def _check_field2neighbors(self):
        set_fields = set(self.fields)
        for field, neighbors in self.field2neighbors.items():
            if field not in set_fields:
                raise ValueError(f'field `{field}` in field2neighbors but not in fields.')
            for neighbor in neighbors:
                if neighbor not in set_fields:
                    raise ValueError(f'field `{neighbor}` in field2neighbors but not in fields.')

    def _num_edges(self):
        return sum(len(neighbors) for neighbors in self.field2neighbors.values())

    def _generate_indices(self):
        """Ascending-sorted [neighbor_idx, field_idx] pairs: W[neighbor_idx, field_idx] of the reference's (F, F) matrix, i.e. an edge
        from the neighbour (source) into the field (destination).  Weight k belongs to pair k."""
        indices = []
        for idx, field in enumerate(self.fields):
            for neighbor in self.field2neighbors.get(field, []):
                indices.append([self.field2idx[neighbor], idx])
        return sorted(indices)

    def _num_sets_of_gnn_weights(self):
        return 1 if self.share_weights_between_layers else self.num_layers

    def build(self, input_shape):
        """Creates `weights_{idx}` (E,) per weight set and the edge tables."""
        if self.built:
            return
        self.indices = self._generate_indices()
        for a, b in zip(self.indices, self.indices[1:]):
            if a == b:       # the reference fails on this inside tf.sparse.to_dense
                raise ValueError('field `%s` lists neighbor `%s` more than once.' % (self.fields[a[1]], self.fields[a[0]]))
        num_edges = self._num_edges()
        self.gnn_weights = [self.add_weight(name=f'weights_{idx}', shape=[num_edges], initializer=self.weights_initializer,
                                            trainable=self.trainable)
                            for idx in range(self._num_sets_of_gnn_weights())]
        self.edge_tables = edge_tables(self.indices, len(self.fields))
        self._tab = tuple(_pack_tables(self.edge_tables, len(self.fields)))
        self._edges = tuple(s for s, _ in self.indices) + tuple(d for _, d in self.indices) or (0,)     # the dense route's src | dst
        self.built = True

    def chosen_route(self):
        """'edges' or 'dense': what `route` comes to for this graph."""
        if self.route != 'auto':
            return self.route
        return auto_route(len(self.fields), self._num_edges())

    def _plan_inputs(self, inputs):
        """(tensors, layout) of the kernel call.  Shape errors first, as the reference raises them; then the device check."""
        F = len(self.fields)
        if isinstance(inputs, (list, tuple)):
            xs = list(inputs)
            if len(xs) == F and all(isinstance(x, torch.Tensor) and x.dim() == 2 and x.shape == xs[0].shape for x in xs):
                for x in xs:
                    _lib.require_gpu(x, 'SparseGNNLayer input')
                return xs, LAYOUT_LIST
            inputs = torch.cat(xs, dim=-1)              # unequal widths or another count: the reference's concat, then its 2-D rule
        if not isinstance(inputs, torch.Tensor):
            raise TypeError('SparseGNNLayer input must be a torch.Tensor or a list of them, got %s' % type(inputs))
        if inputs.dim() == 2:
            if inputs.shape[-1] % F != 0:
                raise ValueError(f'can not determine embedding_dim! {inputs.shape[-1]} can not be divided by {F}.')
            layout = LAYOUT_BFD
        elif inputs.dim() != 3:
            raise ValueError('SparseGNNLayer expects (B, F, D), (B, D, F), (B, F*D) or a list of F (B, D) tensors, got shape %s'
                             % (tuple(inputs.shape),))
        elif inputs.shape[1] == F:
            if inputs.shape[1] == inputs.shape[2]:
                logging.warning(f'WARNING: #fields and embedding_dim are both {inputs.shape[1]}, treat the input as (B, F, D) format.')
            layout = LAYOUT_BFD
        elif inputs.shape[2] == F:
            layout = LAYOUT_BDF
        else:
            raise ValueError('neither axis of the %s input equals the number of fields (%d)' % (tuple(inputs.shape), F))
        _lib.require_gpu(inputs, 'SparseGNNLayer input')
        return [inputs], layout

    def call(self, inputs, return_all_layers=False, transpose_outputs=True, flattern_outputs=True):
        """inputs: (B, F, D), (B, D, F), (B, F*D) or a list of F tensors (B, D); a 3-D input with F == D is taken as (B, F, D).
        Returns the last layer's output, or with return_all_layers a list of every layer's.  Defaults give (B, F*D);
        transpose_outputs=False gives the (B, D, F) order, flattern_outputs=False keeps three dimensions."""
        F, L = len(self.fields), self.num_layers
        xs, in_layout = self._plan_inputs(inputs)
        dense = self.chosen_route() == 'dense'
        if not dense and F > MAX_FIELDS:
            raise NotImplementedError("SparseGNNLayer: %d fields; the fused kernel holds at most %d (csrc/sparse_gnn.hip); pass route='dense' "
                                      'for up to %d' % (F, MAX_FIELDS, MAX_FIELDS_DENSE))
        if dense and F > MAX_FIELDS_DENSE:
            raise NotImplementedError('SparseGNNLayer: %d fields; the dense route holds at most %d (csrc/sparse_gnn_dense.hip)'
                                      % (F, MAX_FIELDS_DENSE))
        tab = self._edges if dense else self._tab
        out_layout = LAYOUT_BFD if transpose_outputs else LAYOUT_BDF
        E, n_sets = len(self.indices), len(self.gnn_weights)
        if self.act_callable is None:
            w = torch.stack(self.gnn_weights) if n_sets > 1 else self.gnn_weights[0].reshape(1, E)
            meta = (F, E, L, n_sets, self.act_code, in_layout, out_layout, bool(return_all_layers), tab, dense)
            outs = list(_SparseGNNFunction.apply(meta, w, *xs))
        else:       # the kernel runs one linear layer at a time, the callable is torch's
            outs, cur, layout = [], xs, in_layout
            for i in range(L):
                meta = (F, E, 1, 1, 0, layout, out_layout, False, tab, dense)
                z = _SparseGNNFunction.apply(meta, self.gnn_weights[i % n_sets].reshape(1, E), *cur)[0]
                z = self.act_callable(z)
                outs.append(z)
                cur, layout = [z], out_layout
            if not return_all_layers:
                outs = outs[-1:]
        if flattern_outputs:
            outs = [o.reshape(o.shape[0], o.shape[1] * o.shape[2]) for o in outs]
        return outs if return_all_layers else outs[0]

    @staticmethod
    def list_of_edge_to_neighbors(list_of_edge, directed=True):
        """List of (node_to, node_from) pairs -> dict node -> set of neighbours, for the constructor; node_to aggregates node_from.
        directed=False adds the reverse of every pair."""
        field2neighbors = {}

        def add_pair(node_to, node_from):
            field2neighbors.setdefault(node_to, set()).add(node_from)

        for pair in list_of_edge:
            add_pair(pair[0], pair[1])
            if not directed:
                add_pair(pair[1], pair[0])
        return field2neighbors
