"""CPU: the fp64 oracle of tests/_tensor_util_oracle.py reproduces the reference's own unit-test cases (tests/golden/tensor_util.npz); the host side
of PoolingLayer, pad_or_truncate / FixLengthLayer and the element-wise embedding weights refuses what it documents to refuse, before any launch;
the CSR inverse of a position table."""
import numpy as np
import pytest
import torch

import _tensor_util_oracle as O


def test_oracle_reproduces_the_reference_cases(golden):
    g = golden('tensor_util')
    assert np.array_equal(O.reduce_axis(g['pool_in'], 0, True, 'sum'), g['pool_axis0_keepdims_sum'])
    assert np.array_equal(O.reduce_axis(g['pool_in'], 1, False, 'sum'), g['pool_axis1_sum'])
    length, axis = int(g['fix_length']), int(g['fix_axis'])
    for case in ('truncate', 'pad', 'same'):
        got = O.pad_or_truncate(g['fix_%s_in' % case], length, axis, 0)
        assert got.dtype == np.float32 and np.array_equal(got, g['fix_%s_out' % case]), case
    pos = g['elw_pos_idx'].tolist()
    assert pos == [0, 1, 1, 2, 2, 2] and g['elw_weights'].shape == (4, 3)
    assert np.array_equal(O.gather_weight(g['elw_weights'], pos), g['elw_out'])


def test_oracle_gradients_on_hand_cases():
    x = np.array([[1., 3., 3.], [2., 2., 2.]])
    g = np.array([6., 9.])
    assert np.array_equal(O.reduce_axis_grad(x, 1, False, 'max', g), [[0., 3., 3.], [3., 3., 3.]])
    assert np.array_equal(O.reduce_axis_grad(x, 1, False, 'min', g), [[6., 0., 0.], [3., 3., 3.]])
    assert np.array_equal(O.reduce_axis_grad(x, -1, True, 'mean', g.reshape(2, 1)), [[2., 2., 2.], [3., 3., 3.]])
    assert np.array_equal(O.reduce_axis_grad(x, None, False, 'sum', np.array(5.)), np.full((2, 3), 5.))
    assert np.array_equal(O.pad_or_truncate_grad((2, 3), 2, -1, np.ones((2, 2))), [[1., 1., 0.], [1., 1., 0.]])
    assert np.array_equal(O.pad_or_truncate_grad((2, 1), 3, 1, np.arange(6.).reshape(2, 3)), [[0.], [3.]])
    dw, dx = O.elem_weight_grads(np.full((1, 3), 2.), np.array([[10., 20.]]), [1, 0, 1], np.array([[1., 2., 4.]]))
    assert np.array_equal(dw, [[4., 10.]]) and np.array_equal(dx, [[20., 20., 80.]])


def test_csr_inverse_of_a_position_table():
    """A table with a repeated (2), an absent (1) and an unsorted (0 after 2) embedding."""
    from rec_now_amd.rec_block.embedding_wise_weight import _csr_inverse
    pos, E = [2, 0, 2, 3, 0, 2], 5
    off, idx = _csr_inverse(pos, E)
    assert off == [0, 2, 2, 5, 6, 6] and idx == [1, 4, 0, 2, 5, 3]
    assert (off, idx) == O.csr_inverse(pos, E)
    for e in range(E):
        assert [p for p in range(len(pos)) if pos[p] == e] == idx[off[e]:off[e + 1]]
    assert _csr_inverse([], 3) == ([0, 0, 0, 0], [])
    rng = np.random.default_rng(0)
    pos = rng.integers(0, 40, 300).tolist()
    assert _csr_inverse(pos, 40) == O.csr_inverse(pos, 40)


def test_pooling_layer_arguments():
    from rec_now_amd.layers import PoolingLayer
    from rec_now_amd.layers.pooling_layer import _fold
    x = torch.zeros(2, 3, 4, 5)
    assert PoolingLayer()(x) is x                                                        # combiner=None returns the input
    assert PoolingLayer(combiner=lambda t: t.shape)(x) == x.shape                        # a callable is called on the input
    with pytest.raises(ValueError, match="combiner must be one of None, 'mean', 'sum', 'max', 'min' or a callable object"):
        PoolingLayer(combiner='median')(x)
    assert set(PoolingLayer.combiner_to_func) == {'mean', 'sum', 'max', 'min'}
    assert _fold((2, 3, 4, 5), 1) == ([1], 2, 3, 20) and _fold((2, 3, 4, 5), -1) == ([3], 24, 5, 1)
    assert _fold((2, 3, 4, 5), None) == ([0, 1, 2, 3], 1, 120, 1) and _fold((2, 3, 4, 5), (2, 1)) == ([1, 2], 2, 12, 5)
    assert _fold((2, 3, 4, 5), [0]) == ([0], 1, 2, 60)
    with pytest.raises(NotImplementedError, match=r'\[0, 2\]'):
        PoolingLayer(axis=[0, 2], combiner='sum')(x)
    with pytest.raises(NotImplementedError):
        PoolingLayer(axis=(1, 1), combiner='sum')(x)
    with pytest.raises(ValueError, match='out of range'):
        PoolingLayer(axis=4, combiner='sum')(x)
    with pytest.raises(ValueError, match='empty axis'):
        PoolingLayer(axis=1, combiner='max')(torch.zeros(2, 0, 3))
    with pytest.raises(TypeError, match='float64'):
        PoolingLayer(axis=1, combiner='sum')(x.double())
    with pytest.raises(TypeError, match='int64'):
        PoolingLayer(axis=1, combiner='sum')(x.long())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        PoolingLayer(axis=1, combiner='sum')(x)


def test_fix_length_arguments():
    from rec_now_amd.layers import FixLengthLayer
    from rec_now_amd.layers.fix_length_layer import _fill_bits, pad_or_truncate
    x = torch.zeros(2, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pad_or_truncate(x, 5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        FixLengthLayer(length=2, axis=-1, name='FixLengthLayer')(x)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pad_or_truncate(x, 3)                                                            # the equal length too: the input stays a GPU tensor
    with pytest.raises(TypeError, match='float16'):
        pad_or_truncate(x.half(), 5)
    with pytest.raises(ValueError, match='out of range'):
        pad_or_truncate(x, 5, axis=2)
    with pytest.raises(ValueError, match='length'):
        pad_or_truncate(x, -1)
    assert _fill_bits(0, torch.float32) == 0 and _fill_bits(1.5, torch.float32) == 0x3fc00000
    assert _fill_bits(-1, torch.int32) == 0xffffffff and _fill_bits(-1, torch.int64) == -1 and _fill_bits(7, torch.int64) == 7
    layer = FixLengthLayer(4, 1, constant_values=9)
    assert (layer.length, layer.axis, layer.constant_values) == (4, 1, 9)


def test_element_wise_weight_arguments():
    from rec_now_amd.rec_block.embedding_wise_weight import (_position_table, apply_embedding_element_wise_weight,
                                                             gather_embedding_element_wise_weight)
    w = torch.zeros(4, 3)
    for table in ([0, 1, 1, 2], (0, 1, 1, 2), np.array([0, 1, 1, 2]), np.array([[0, 1, 1, 2]]), torch.tensor([0, 1, 1, 2]), torch.tensor([[0, 1, 1, 2]])):
        assert _position_table(table, 3) == (0, 1, 1, 2)
    assert _position_table([], 3) == ()
    with pytest.raises(ValueError, match=r'\[0, 3\)'):
        gather_embedding_element_wise_weight(w, [0, 3])
    with pytest.raises(ValueError, match=r'\[0, 3\)'):
        gather_embedding_element_wise_weight(w, [-1, 0])
    with pytest.raises(NotImplementedError, match=r'\(4, 2\)'):
        gather_embedding_element_wise_weight(w, np.zeros((4, 2), dtype=np.int64))
    with pytest.raises(TypeError):
        gather_embedding_element_wise_weight(w, [0.5, 1.0])
    with pytest.raises(ValueError, match='rank'):
        gather_embedding_element_wise_weight(torch.zeros(3), [0])
    with pytest.raises(ValueError, match='inputs must be'):
        apply_embedding_element_wise_weight(torch.zeros(4, 5), w, [0, 1, 2])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        gather_embedding_element_wise_weight(w, [0, 1, 2])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        apply_embedding_element_wise_weight(torch.zeros(4, 3), w, [0, 1, 2])
