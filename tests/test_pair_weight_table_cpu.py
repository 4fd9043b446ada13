"""CPU: LabelPairWeightTable of rec_now_amd.rec_block.pairwise_loss_from_batch -- how the K x K table is built (explicit weights, one
call of the weight function on the broadcast value matrices, the default rule), the table as an ordinary weight callable, and every
argument it refuses.  Bit for bit: a table entry IS the function's float32 value at that pair of label values."""
import numpy as np
import pytest
import torch


def _mod():
    from rec_now_amd.rec_block import pairwise_loss_from_batch as M
    return M


def _gap(a, b, **k):
    return torch.clamp(a - b, min=0.0) * k.get('scale', 1.0)


def _sym(a, b, **k):
    return (a - b).abs() + 0.5


VALUES = [0.0, 1.0, 1.1, 3.0, -2.5]


@pytest.mark.parametrize('func,kwargs', [(_gap, {'scale': 2.0}), (_gap, {}), (_sym, {})])
def test_table_is_the_function_on_the_value_matrices(func, kwargs):
    M = _mod()
    t = M.LabelPairWeightTable(VALUES, func, **kwargs)
    v = torch.tensor(VALUES, dtype=torch.float32)
    a, b = v.reshape(-1, 1).expand(5, 5), v.reshape(1, -1).expand(5, 5)
    want = func(a, b, **kwargs)
    assert t.n_values == 5 and t.weights.dtype == torch.float32 and t.label_values.dtype == torch.float32
    assert torch.equal(t.label_values, v)
    assert torch.equal(t.weights, want)
    # W[a, b]: positive row values[a], negative row values[b]
    assert t.weights[3, 0].item() == func(torch.tensor(3.0), torch.tensor(0.0), **kwargs).item()


def test_values_from_numpy_and_tensor_are_compared_as_float32():
    M = _mod()
    t = M.LabelPairWeightTable(np.array([0.0, 1.1, 2.0], dtype=np.float64), _sym)
    assert torch.equal(t.label_values, torch.tensor([0.0, 1.1, 2.0], dtype=torch.float32))
    t2 = M.LabelPairWeightTable(torch.tensor([0, 1, 2], dtype=torch.int64), _sym)
    assert torch.equal(t2.weights, torch.tensor([[0.5, 1.5, 2.5], [1.5, 0.5, 1.5], [2.5, 1.5, 0.5]]))


@pytest.mark.parametrize('func,kwargs', [(_gap, {'scale': 2.0}), (_sym, {})])
def test_callable_returns_the_functions_weights(func, kwargs):
    M = _mod()
    t = M.LabelPairWeightTable(VALUES, func, **kwargs)
    rng = np.random.default_rng(5)
    v = np.array(VALUES, dtype=np.float32)
    lp = torch.from_numpy(v[rng.integers(0, 5, 4096)])
    ln = torch.from_numpy(v[rng.integers(0, 5, 4096)])
    got = t(lp, ln, anything='ignored')
    assert got.dtype == torch.float32 and got.shape == lp.shape
    assert torch.equal(got, func(lp, ln, **kwargs))
    # (P, 1) x (1, P) label matrices, as the dense formulation passes them
    assert torch.equal(t(lp[:7].reshape(-1, 1), ln[:9].reshape(1, -1)), func(lp[:7].reshape(-1, 1), ln[:9].reshape(1, -1), **kwargs))
    # float64 labels holding the same float32 values look up the same entries
    assert torch.equal(t(lp.double(), ln.double()), got)


def test_callable_gives_nan_for_a_foreign_label():
    M = _mod()
    t = M.LabelPairWeightTable([0.0, 1.0, 2.0], _sym)
    got = t(torch.tensor([1.0, 7.0, 2.0, float('nan'), -0.0]), torch.tensor([0.0, 0.0, 5.0, 1.0, 2.0]))
    assert got[0].item() == 1.5
    assert torch.isnan(got[1]) and torch.isnan(got[2]) and torch.isnan(got[3])
    assert got[4].item() == 2.5                      # -0.0 is the value 0.0


def test_default_rule_and_explicit_weights():
    M = _mod()
    t = M.LabelPairWeightTable([2.0, 0.0, 1.0])
    assert torch.equal(t.weights, torch.tensor([[0., 1., 1.], [0., 0., 0.], [0., 1., 0.]]))
    nan, inf = float('nan'), float('inf')
    w = [[0.0, -1.0, nan], [2.0, 0.25, inf], [-inf, 1.0, 0.0]]
    t = M.LabelPairWeightTable([0, 1, 2], weights=w)
    assert np.array_equal(t.weights.numpy(), np.array(w, dtype=np.float32), equal_nan=True)       # kept as given
    t = M.LabelPairWeightTable([0, 1, 2], weights=np.array(w))
    assert np.array_equal(t.weights.numpy(), np.array(w, dtype=np.float32), equal_nan=True)
    got = t(torch.tensor([1.0, 0.0]), torch.tensor([2.0, 1.0]))
    assert got[0].item() == inf and got[1].item() == -1.0
    one = M.LabelPairWeightTable([4.0], _sym)
    assert torch.equal(one.weights, torch.tensor([[0.5]]))


def test_refused_arguments():
    M = _mod()
    T = M.LabelPairWeightTable
    with pytest.raises(ValueError):
        T([])
    with pytest.raises(ValueError):
        T(list(range(17)))
    T(list(range(16)))                                                  # 16 values are fine
    with pytest.raises(ValueError):
        T([0.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        T([0.0, -0.0, 1.0])                                             # equal as float32
    with pytest.raises(ValueError):
        T(np.array([1.0, 1.0 + 1e-12]))                                 # distinct float64, one float32
    with pytest.raises(ValueError):
        T([0.0, float('nan')])
    with pytest.raises(ValueError):
        T([0.0, float('inf')])
    with pytest.raises(ValueError):
        T(np.array([0.0, 1e300]))                                       # infinite as float32
    with pytest.raises(ValueError):
        T([0.0, 1.0], _sym, weights=[[0.0, 1.0], [1.0, 0.0]])           # both a function and weights
    with pytest.raises(ValueError):
        T([0.0, 1.0], weights=[[0.0, 1.0, 1.0]])                        # not (K, K)


def test_routing_helpers_on_the_host():
    """What decides the route is host logic: the BPR options read off a functools.partial, and the refusal of keyword arguments beside a
    table (the table took its own when it was built)."""
    import functools
    M = _mod()
    assert M._bpr_options(M.bpr_loss_func) == (1.0, True)
    assert M._bpr_options(functools.partial(M.bpr_loss_func, factor=0.7)) == (0.7, True)
    assert M._bpr_options(functools.partial(M.bpr_loss_func, reduce_mean=False, factor=2.0)) == (2.0, False)
    assert M._bpr_options(functools.partial(M.bpr_loss_func, weights=None)) is None
    assert M._bpr_options(functools.partial(M.bpr_loss_func, 1.0)) is None
    assert M._bpr_options(lambda p, n, w: M.bpr_loss_func(p, n, w)) is None
    t = M.LabelPairWeightTable([0.0, 1.0])
    z = torch.zeros(4)
    with pytest.raises(ValueError, match='keyword'):
        M.pairwise_loss(z, z, z, label_pair_to_weight_func=t, scale=2.0)
