"""CPU: the fp64 oracle of StarDense / StackedDense (tests/_star_oracle.py) against the reference's four goldens, and the host side of
the layers (signatures, variable names and shapes, class methods, argument errors) without a GPU."""
import inspect

import numpy as np
import pytest
import torch

import _star_oracle as S
import dense_ref as R

T = lambda a: torch.from_numpy(np.asarray(a)).double()      # noqa: E731
TOL = 1e-5


def keras_adam(params, grads, state, t, lr=0.005, beta1=0.9, beta2=0.999, eps=1e-7):
    """One tf.keras.optimizers.Adam step (bias correction folded into the step size, eps outside the square root), in place."""
    step = lr * (1 - beta2 ** t) ** 0.5 / (1 - beta1 ** t)
    with torch.no_grad():
        for p, g in zip(params, grads):
            m, v = state.setdefault(id(p), (torch.zeros_like(p), torch.zeros_like(p)))
            m.mul_(beta1).add_((1 - beta1) * g)
            v.mul_(beta2).add_((1 - beta2) * g * g)
            p.sub_(step * m / (v.sqrt() + eps))


def test_oracle_star_dense_golden(golden):
    g = golden('star_dense')
    out = S.star_dense(T(g['inputs']), T(g['kernel']), T(g['bias']), [T(g['params'])])
    assert R.calc_sum_of_abs_diff(out.numpy(), g['golden']) < TOL


def test_oracle_stacked_dense_golden(golden):
    g = golden('stacked_dense')
    out = S.stacked_dense(T(g['inputs']), T(g['kernel']), T(g['bias']), T(g['params']).chunk(1))
    assert R.calc_sum_of_abs_diff(out.numpy(), g['golden']) < TOL


def test_oracle_parasitic_goldens(golden):
    g = golden('parasitic_star')
    pk, pb = torch.ones(5, 3, 4, dtype=torch.float64), torch.zeros(5, 4, dtype=torch.float64)
    for grp in (0, 1):
        out = S.parasitic_dense(T(g['inputs']), T(g['kernel']), T(g['bias']), pk, pb, grp, 'star')
        assert R.calc_sum_of_abs_diff(out.numpy(), g['golden']) < TOL
    g = golden('parasitic_stacked')
    out = S.parasitic_dense(T(g['inputs']), T(g['kernel']), T(g['bias']), torch.ones(1, 2, 3, dtype=torch.float64),
                            torch.zeros(1, 3, dtype=torch.float64), 0, 'stacked')
    assert R.calc_sum_of_abs_diff(out.numpy(), g['golden']) < TOL


def test_oracle_parasitic_adam_golden(golden):
    # reference tests/layers/test_star_dense_layer.py:78-107: three Adam steps on group 1 with the trunk frozen
    g = golden('parasitic_star')
    x, k, b = T(g['grad_inputs']), T(g['grad_kernel']), T(g['grad_bias'])
    pk = torch.ones(2, 3, 1, dtype=torch.float64, requires_grad=True)
    pb = torch.zeros(2, 1, dtype=torch.float64, requires_grad=True)
    state = {}
    for t in (1, 2, 3):
        loss = ((S.parasitic_dense(x, k, b, pk, pb, 1, 'star') - 1.0) ** 2).sum(1).mean()
        keras_adam((pk, pb), torch.autograd.grad(loss, (pk, pb)), state, t)
    assert R.calc_sum_of_abs_diff(pk.detach().numpy(), g['golden_parasitic_kernel']) < TOL
    assert R.calc_sum_of_abs_diff(pb.detach().numpy(), g['golden_parasitic_bias']) < TOL
    assert abs(loss.item() - float(g['golden_loss'])) < TOL


def test_layer_signatures_and_class_methods():
    from rec_now_amd.layers.stacked_dense_layer import ParasiticStackedDenseLayer, StackedDenseLayer
    from rec_now_amd.layers.star_dense_layer import ParasiticStarDenseLayer, StarDenseLayer
    from rec_now_amd.util.param_normalizer import wrap_as_list
    assert list(inspect.signature(StarDenseLayer.call).parameters) == ['self', 'inputs', 'starnet_param_list']
    assert list(inspect.signature(StackedDenseLayer.call).parameters) == ['self', 'inputs', 'resnet_param_list', 'resnet_weight']
    assert inspect.signature(StackedDenseLayer.call).parameters['resnet_weight'].default == 1.0
    for cls, init in ((ParasiticStarDenseLayer, 'Ones'), (ParasiticStackedDenseLayer, 'Zeros')):
        ps = inspect.signature(cls.__init__).parameters
        assert list(ps)[1:7] == ['kernel', 'bias', 'dense_layer', 'activation', 'parasitic_kernel_initializer', 'num_groups']
        assert ps['parasitic_kernel_initializer'].default == init
        assert list(inspect.signature(cls.call).parameters) == ['self', 'inputs', 'group_idx', 'stop_trunk_grad']
    assert StarDenseLayer.get_starnet_param_size(3, 5) == 20 == StackedDenseLayer.get_resnet_param_size(3, 5)
    assert torch.equal(StarDenseLayer.get_starnet_kernel_initializer()((2, 3)), torch.ones(2, 3))
    assert torch.equal(StarDenseLayer.get_starnet_bias_initializer()((4,)), torch.zeros(4))
    assert torch.equal(StackedDenseLayer.get_resnet_kernel_initializer()((2, 3)), torch.zeros(2, 3))
    assert torch.equal(StackedDenseLayer.get_resnet_bias_initializer()((4,)), torch.zeros(4))
    t = torch.zeros(2)
    assert wrap_as_list(t)[0] is t and wrap_as_list([t, t]) == [t, t]


@pytest.mark.parametrize('use_bias', [True, False])
def test_layer_variables(use_bias):
    from rec_now_amd.layers.stacked_dense_layer import StackedDenseLayer
    from rec_now_amd.layers.star_dense_layer import StarDenseLayer
    for cls in (StarDenseLayer, StackedDenseLayer):
        layer = cls(5, use_bias=use_bias)
        layer.build((2, 3))
        shapes = {k: tuple(v.shape) for k, v in layer.named_weights().items()}
        assert shapes == ({'kernel': (3, 5), 'bias': (5,)} if use_bias else {'kernel': (3, 5)})


def test_parasitic_variables_and_trunk_sources():
    from rec_now_amd.layers.stacked_dense_layer import ParasiticStackedDenseLayer
    from rec_now_amd.layers.star_dense_layer import ParasiticStarDenseLayer
    k, b = torch.randn(3, 4), torch.randn(4)
    layer = ParasiticStarDenseLayer(kernel=k, bias=b, num_groups=5)
    layer.build((2, 3))
    w = layer.named_weights()
    assert tuple(w['kernel'].shape) == (5, 3, 4) and tuple(w['bias'].shape) == (5, 4)
    assert torch.equal(w['kernel'], torch.ones(5, 3, 4)) and torch.equal(w['bias'], torch.zeros(5, 4))

    class Trunk:                                     # any object with .kernel / .bias and a lazy build()
        built = False

        def build(self, input_shape):
            self.kernel, self.bias, self.built = torch.randn(input_shape[-1], 2), None, True

    layer = ParasiticStackedDenseLayer(dense_layer=Trunk(), num_groups=2)
    layer.build((7, 6))
    w = layer.named_weights()
    assert list(w) == ['kernel'] and torch.equal(w['kernel'], torch.zeros(2, 6, 2))
    with pytest.raises(ValueError, match='kernel is None'):
        ParasiticStarDenseLayer()


def test_argument_errors_before_any_device_call():
    from rec_now_amd.layers.stacked_dense_layer import StackedDenseLayer
    from rec_now_amd.layers.star_dense_layer import ParasiticStarDenseLayer, StarDenseLayer
    for cls in (StarDenseLayer, StackedDenseLayer):
        layer = cls(5)
        layer.build((2, 3))
        p = torch.ones(2, 20)
        with pytest.raises(ValueError, match=r'\(B, D\) input'):
            layer(torch.zeros(2, 1, 3), p)
        with pytest.raises(ValueError, match='size-incompatible'):
            layer(torch.zeros(2, 4), p)
        with pytest.raises(ValueError, match=r'\(B, D\*U\+U\) = \(2, 20\)'):
            layer(torch.zeros(2, 3), torch.ones(2, 19))
        with pytest.raises(ValueError, match=r'\(B, D\*U\+U\)'):
            layer(torch.zeros(2, 3), [p, torch.ones(3, 20)])
    par = ParasiticStarDenseLayer(kernel=torch.zeros(3, 4))
    with pytest.raises(ValueError, match=r'\(B, D\) input'):
        par(torch.zeros(3))
    with pytest.raises(ValueError, match='size-incompatible'):
        par(torch.zeros(2, 5))
