"""CPU: the host side of CANLayer (rec_now_amd/layers/can_layer.py) -- the fp64 oracle (tests/_can_oracle.py) against the reference's golden,
parameter sizes, the argument errors of the reference, the refusals of this package, and the host-only shape query of csrc/can.hip."""
import ctypes

import numpy as np
import pytest
import torch

import _can_oracle as C


def _layer(**kw):
    from rec_now_amd.layers.can_layer import CANLayer
    return CANLayer(**kw)


def test_oracle_reproduces_the_reference_golden(golden):
    # reference tests/layers/test_can_layer.py:27-51
    from rec_now_amd.util.numpy_tools import calc_sum_of_abs_diff
    g = golden('can')
    got = C.can_layer(torch.from_numpy(g['inputs']).double(), torch.from_numpy(g['params']).double(), g['dims'].tolist())
    assert calc_sum_of_abs_diff(got, g['golden']) < 1e-5


def test_has_non_zero_golden(golden):
    # reference tests/layers/test_can_layer.py:18-25
    from rec_now_amd.layers import CANLayer
    g = golden('can')
    got = CANLayer._has_non_zero(torch.from_numpy(g['nz_inputs']), axis=-1, keepdims=True)
    assert got.dtype == torch.bool and got.shape == (2, 2, 1)
    assert np.array_equal(got.numpy(), g['nz_golden'])
    assert not CANLayer._has_non_zero(torch.tensor([[-0.0, 0.0]]), keepdims=False).item()           # -0.0 is zero


def test_param_sizes():
    from rec_now_amd.layers.can_layer import CANLayer
    assert CANLayer.CAN_EXPANDED_INPUT_DIM == 4
    assert CANLayer.get_dnn_param_size(4, [4, 3, 2]) == 43 == C.param_size(4, [4, 3, 2])
    assert CANLayer.get_dnn_param_size(4, [4, 3, 2], use_bias=False) == 34
    assert CANLayer._get_layer_param_size(5, 7, True) == 42 and CANLayer._get_layer_param_size(5, 7, False) == 35


def test_auto_decided_dims():
    layer = _layer(dnn_dims=None)
    for d0, n in ((4, 1), (4, 8), (16, 3)):
        assert layer._auto_decide_dnn_param_size(d0, n * (d0 * d0 + d0)) == [d0] * n
    assert _layer(dnn_dims=None, use_bias=False)._auto_decide_dnn_param_size(4, 32) == [4, 4]
    with pytest.raises(ValueError, match='dnn_param_size not match'):
        layer._auto_decide_dnn_param_size(4, 43)
    with pytest.raises(ValueError, match='dnn_param_size not match'):       # through call, before any device is asked for
        layer(torch.zeros(2, 3, 4), torch.zeros(2, 43))


def test_param_size_mismatch_raises():
    with pytest.raises(ValueError, match='dnn_param_size not match'):
        _layer(dnn_dims=[4, 3, 2])(torch.zeros(2, 3, 4), torch.zeros(2, 42))
    with pytest.raises(ValueError, match='dnn_param_size not match'):
        _layer(dnn_dims=[4, 3, 2], use_bias=False)(torch.zeros(2, 3, 4), torch.zeros(2, 43))
    _layer(dnn_dims=[4, 3, 2])._check_dnn_param_size(4, [4, 3, 2], 43)


def test_res_net_needs_equal_dims():
    with pytest.raises(ValueError, match='use_res_net'):
        _layer(dnn_dims=[4, 3], use_res_net=True)(torch.zeros(2, 3, 4), torch.zeros(2, 35))


def test_activations():
    from rec_now_amd.layers import _keras as K
    for a, code in ((None, K.ACT_LINEAR), ('linear', K.ACT_LINEAR), ('relu', K.ACT_RELU), ('tanh', K.ACT_TANH), ('sigmoid', K.ACT_SIGMOID),
                    (torch.tanh, K.ACT_TANH), (torch.relu, K.ACT_RELU), (torch.sigmoid, K.ACT_SIGMOID)):
        assert _layer(activation=a).act_code == code
    assert _layer().act_code == K.ACT_TANH                                   # the reference's default is tf.tanh
    with pytest.raises(NotImplementedError, match='relu, tanh or sigmoid'):
        _layer(activation=torch.nn.functional.gelu)
    with pytest.raises(NotImplementedError, match='relu, tanh or sigmoid'):
        _layer(activation=lambda v: v)
    with pytest.raises(ValueError):
        _layer(output_combiner='median')


def test_cpu_tensor_and_dtype_are_refused():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _layer(dnn_dims=[4, 3, 2])(torch.zeros(2, 3, 4), torch.zeros(2, 43))
    with pytest.raises(TypeError, match='float32'):
        _layer(dnn_dims=[4, 3, 2])(torch.zeros(2, 3, 4, dtype=torch.float64), torch.zeros(2, 43))
    with pytest.raises(ValueError, match='empty axis'):
        _layer(dnn_dims=[4])(torch.zeros(2, 0, 4), torch.zeros(2, 20))


def _supported(d0, dims, use_bias=1):
    from rec_now_amd import _lib
    return _lib.load().recnow_can_supported(d0, (ctypes.c_int * len(dims))(*dims), len(dims), use_bias)


def test_supported_shapes():
    from rec_now_amd.layers.can_layer import can_supported
    assert _supported(64, [64, 64]) == 1
    assert _supported(4, [4, 3, 2]) == 1 and _supported(1, [1]) == 1 and _supported(4, [4] * 8) == 1
    assert _supported(16, [16, 16]) == 1 and _supported(32, [32, 32, 32]) == 1
    assert _supported(64, [65, 64]) == 0 and _supported(65, [64]) == 0 and _supported(64, [64, 65]) == 0       # a dim of 65
    assert _supported(4, [4] * 9) == 0                                                                     # 9 layers
    assert _supported(4, [4, 0, 2]) == 0 and _supported(0, [4]) == 0                                       # a dim of 0
    assert _supported(4, [], 1) == 0
    assert _supported(64, [64] * 8) == 0                             # 33 280 parameters: more than the 64 KB of LDS a workgroup asks for
    assert can_supported(64, [64, 64]) and not can_supported(64, [65])


def test_unsupported_shape_is_named(monkeypatch):
    from rec_now_amd import _lib
    from rec_now_amd.layers.can_layer import CANLayer
    monkeypatch.setattr(_lib, 'require_gpu', lambda t, what='tensor': t)     # reach the shape check without a device
    with pytest.raises(NotImplementedError, match=r'1\.\.64'):
        CANLayer(dnn_dims=[65])(torch.zeros(2, 3, 4), torch.zeros(2, CANLayer.get_dnn_param_size(4, [65])))
    with pytest.raises(NotImplementedError, match=r'1\.\.8 layers'):
        CANLayer(dnn_dims=None)(torch.zeros(2, 3, 4), torch.zeros(2, 9 * 20))
