"""CPU: SparseGNNLayer's host side (rec_now_amd/layers/sparse_gnn_layer.py) and its fp64 oracle (tests/_gnn_oracle.py): the reference
golden through the oracle, the weight order as literals, a hand-computed case with distinct weights, list_of_edge_to_neighbors,
every validation error, weight names and shapes, and the kernel's edge tables.  No kernel runs here."""
import numpy as np
import pytest
import torch

import _gnn_oracle as G
from rec_now_amd.layers.sparse_gnn_layer import SparseGNNLayer, edge_tables

DOC_FIELDS = ['user_id', 'user_age', 'doc_id', 'doc_subject']
DOC_NEIGHBORS = {'user_id': ['doc_id', 'doc_subject'], 'user_age': ['doc_subject'], 'doc_subject': ['user_age']}


def _built(*args, **kw):
    layer = SparseGNNLayer(*args, **kw)
    layer.build(None)
    return layer


def test_fixture_against_the_oracle(golden):
    # reference tests/layers/test_sparse_gnn_layer.py:19-47
    g = golden('sparse_gnn')
    indices = g['indices'].tolist()
    weights = [torch.full((len(indices),), float(g['weight']), dtype=torch.float64) for _ in range(int(g['num_layers']))]
    got = G.sparse_gnn_bfd(torch.from_numpy(g['inputs']).double(), indices, weights, int(g['num_layers']), 'tanh')[-1]
    assert np.abs(got.numpy() - g['golden']).sum() < 1e-5
    layer = _built([0, 1, 2], {0: [2], 1: [2, 0]}, num_layers=3, share_weights_between_layers=False)
    assert layer.indices == indices


def test_index_order_of_the_docstring_example():
    # reference sparse_gnn_layer.py:25-55; entry k of a weight vector belongs to pair k of this list
    assert G.sorted_indices(DOC_FIELDS, DOC_NEIGHBORS) == [[1, 3], [2, 0], [3, 0], [3, 1]]
    layer = _built(DOC_FIELDS, DOC_NEIGHBORS, num_layers=3, share_weights_between_layers=False, activation='tanh')
    assert layer.indices == [[1, 3], [2, 0], [3, 0], [3, 1]]


def test_oracle_with_distinct_weights_by_hand():
    """Two fields, D = 1, linear: field a aggregates b with weight for pair [1, 0], b aggregates a with weight for pair [0, 1].
    Sorted pairs: [[0, 1], [1, 0]], so w[0] is a -> b (added to b) and w[1] is b -> a (added to a).  x = (a, b) = (2, 3), w = (10, 100):
    a' = 2 + 100 * 3 = 302,  b' = 3 + 10 * 2 = 23.  Swapped weights would give (32, 203)."""
    indices = G.sorted_indices(['a', 'b'], {'a': ['b'], 'b': ['a']})
    assert indices == [[0, 1], [1, 0]]
    x = torch.tensor([[[2.0, 3.0]]], dtype=torch.float64)                  # (B, D, F)
    w = torch.tensor([10.0, 100.0], dtype=torch.float64)
    out = G.sparse_gnn(x, indices, [w], 1, 'linear')[0]
    assert out.tolist() == [[[302.0, 23.0]]]
    out2 = G.sparse_gnn(x, indices, [w], 2, 'linear')[1]                   # a'' = 302 + 100 * 23, b'' = 23 + 10 * 302
    assert out2.tolist() == [[[2602.0, 3043.0]]]


def test_list_of_edge_to_neighbors():
    # reference tests/layers/test_sparse_gnn_layer.py:64-83
    edges = [(1, 2), (1, 3), (2, 3)]
    assert SparseGNNLayer.list_of_edge_to_neighbors(edges, directed=True) == {1: {2, 3}, 2: {3}}
    assert SparseGNNLayer.list_of_edge_to_neighbors(edges, directed=False) == {1: {2, 3}, 2: {1, 3}, 3: {1, 2}}
    assert SparseGNNLayer.list_of_edge_to_neighbors(edges) == {1: {2, 3}, 2: {3}}


def test_pairs_and_sets_as_field2neighbors():
    a = _built([1, 2, 3], [(1, 2), (1, 3), (2, 3)])
    b = _built([1, 2, 3], {(1, 2), (1, 3), (2, 3)})
    c = _built([1, 2, 3], {1: {2, 3}, 2: {3}})
    assert a.indices == b.indices == c.indices == [[1, 0], [2, 0], [2, 1]]


def test_validation_errors():
    with pytest.raises(ValueError, match='duplicated fields'):
        SparseGNNLayer(['a', 'b', 'a'], {})
    with pytest.raises(ValueError, match='`c` in field2neighbors but not in fields'):
        SparseGNNLayer(['a', 'b'], {'c': ['a']})
    with pytest.raises(ValueError, match='`c` in field2neighbors but not in fields'):
        SparseGNNLayer(['a', 'b'], {'a': ['c']})
    with pytest.raises(TypeError, match='field2neighbors must be one of'):
        SparseGNNLayer(['a', 'b'], (('a', 'b'),))
    with pytest.raises(TypeError, match='field2neighbors must be one of'):
        SparseGNNLayer(['a', 'b'], 'ab')
    with pytest.raises(ValueError, match='more than once'):
        SparseGNNLayer(['a', 'b'], {'a': ['b', 'b']})(torch.zeros(2, 2, 4))
    layer = SparseGNNLayer(['a', 'b', 'c'], {'a': ['b']})
    with pytest.raises(ValueError, match='can not be divided by 3'):
        layer(torch.zeros(2, 10))
    with pytest.raises(ValueError, match='neither axis'):
        layer(torch.zeros(2, 4, 5))
    with pytest.raises(ValueError, match='Unknown activation'):
        SparseGNNLayer(['a', 'b'], {}, activation='gelu')


def test_cpu_tensor_is_refused():
    layer = SparseGNNLayer(['a', 'b', 'c'], {'a': ['b']})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        layer(torch.zeros(2, 3, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        layer([torch.zeros(2, 4)] * 3)


def test_square_input_is_taken_as_bfd(caplog):
    layer = SparseGNNLayer(['a', 'b', 'c'], {'a': ['b']})
    layer.build(None)
    with caplog.at_level('WARNING'):
        with pytest.raises(RuntimeError, match='no CPU fallback'):       # past the shape rule, at the device check
            layer(torch.zeros(2, 3, 3))
    assert 'treat the input as (B, F, D) format' in caplog.text


@pytest.mark.parametrize('share,n_sets', [(True, 1), (False, 3)])
def test_weight_names_and_shapes(share, n_sets):
    layer = _built(DOC_FIELDS, DOC_NEIGHBORS, num_layers=3, share_weights_between_layers=share)
    w = layer.named_weights()
    assert sorted(w) == ['weights_%d' % i for i in range(n_sets)]
    for v in w.values():
        assert tuple(v.shape) == (4,) and v.requires_grad
        assert torch.equal(v.detach(), torch.full((4,), 0.1))            # the default initializer: constant 0.1
    frozen = _built(DOC_FIELDS, DOC_NEIGHBORS, num_layers=2, share_weights_between_layers=False, trainable=False)
    assert all(not v.requires_grad for v in frozen.named_weights().values())
    ones = _built(DOC_FIELDS, DOC_NEIGHBORS, weights_initializer='ones')
    assert torch.equal(ones.named_weights()['weights_0'].detach(), torch.ones(4))


def test_edge_tables_are_permutations_of_one_edge_list():
    rng = np.random.default_rng(3)
    for F, E in ((4, 4), (7, 0), (5, 25), (9, 30)):
        flat = rng.permutation(F * F)[:E]
        indices = sorted([int(p // F), int(p % F)] for p in flat)
        t = edge_tables(indices, F)
        for ptr, col, wid, other in (('dptr', 'dsrc', 'dwid', 1), ('sptr', 'sdst', 'swid', 0)):
            assert len(t[ptr]) == F + 1 and t[ptr][0] == 0 and t[ptr][-1] == E
            assert sorted(t[wid]) == list(range(E))                      # every weight index exactly once
            for i in range(F):
                for k in range(t[ptr][i], t[ptr][i + 1]):
                    e = indices[t[wid][k]]
                    assert e[other] == i and e[1 - other] == t[col][k]      # entry k is edge wid[k]: segment node and other end
        assert [indices[k][0] for k in t['swid']] == t['ssrc']
        assert t['swid'] == list(range(E))                               # sorted [src, dst] order IS the by-source order
    doc = edge_tables([[1, 3], [2, 0], [3, 0], [3, 1]], 4)
    assert doc['dptr'] == [0, 2, 3, 3, 4] and doc['dsrc'] == [2, 3, 3, 1] and doc['dwid'] == [1, 2, 3, 0]
    assert doc['sptr'] == [0, 0, 1, 2, 4] and doc['sdst'] == [3, 0, 0, 1]
