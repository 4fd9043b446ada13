"""GPU: CANLayer (csrc/can.hip) against the reference's golden and against the fp64 oracle (tests/_can_oracle.py): y, dx and dparams over a
pruned shape / option sweep, the tie rule of max / min, bit-identical runs, a captured graph, and the forward's memory.
Tolerance: 1e-5 relative to the largest magnitude of the compared tensor, the close() of tests/test_star_dense_gpu.py.  Inputs have
unit-variance rows and parameters of std 1 / sqrt(din), so the pre-activations are of O(1)."""
import os
import re

import numpy as np
import pytest
import torch

import _can_oracle as C

pytestmark = pytest.mark.gpu
RTOL = 1e-5


def _positions_per_pass(widest):
    """Positions a workgroup takes per forward pass = per backward chunk, from the constants of csrc/can.hip."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rec_now_amd', 'csrc', 'can.hip')).read()
    threads = int(re.search(r'#define CAN_THREADS (\d+)', src).group(1))
    group = int(re.search(r'#define CAN_MIN_GROUP (\d+)', src).group(1))
    while group < widest:
        group *= 2
    return threads // group


def close(a, b, rtol=RTOL, what=''):
    a, b = a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(np.abs(b).max(), 1e-30) if b.size else 1.0
    err = np.abs(a - b).max() if b.size else 0.0
    print('%s: max err %.3g vs scale %.3g (rel %.3g)' % (what, err, scale, err / scale))
    assert err <= rtol * scale, '%s: max err %.3g vs scale %.3g (rel %.3g)' % (what, err, scale, err / scale)


def _layer(**kw):
    from rec_now_amd.layers import CANLayer
    return CANLayer(**kw)


def _draw(gen, B, L, D0, dims, use_bias, special=True):
    """fp64 (inputs (B, L, D0), params (B, P)); with `special`: some all-zero rows, one row of -0.0, one sample of zero rows only."""
    x = torch.randn(B, L, D0, generator=gen, dtype=torch.float64)
    parts, din = [], D0
    for dout in dims:
        parts.append(torch.randn(B, din * dout, generator=gen, dtype=torch.float64) / din ** 0.5)
        if use_bias:
            parts.append(torch.randn(B, dout, generator=gen, dtype=torch.float64) * 0.5)
        din = dout
    if special:
        x[torch.rand(B, L, generator=gen) < 0.25] = 0.0
        x[0, L - 1] = -0.0
        if B > 1:
            x[B - 1] = 0.0
    return x, torch.cat(parts, 1)


def test_reference_golden(dev, golden):
    # reference tests/layers/test_can_layer.py:27-51
    from rec_now_amd.util.numpy_tools import calc_sum_of_abs_diff
    g = golden('can')
    x, p = torch.from_numpy(g['inputs']).to(dev), torch.from_numpy(g['params']).to(dev)
    out = _layer(dnn_dims=g['dims'].tolist(), use_bias=True, mask_all_zero_embedding=True)(x, p)
    assert calc_sum_of_abs_diff(out.cpu(), g['golden']) < 1e-5
    assert calc_sum_of_abs_diff(_layer(dnn_dims=g['dims'].tolist(), activation=torch.tanh)(x, p).cpu(), g['golden']) < 1e-5


# ---- parity sweep against fp64 ---------------------------------------------------------------------------------
def _first_half(v):
    return v[:, : (v.shape[1] + 1) // 2].sum(1)


C16 = _positions_per_pass(16)
# B, L (None: a (B, D0) input), D0, dims, pass dnn_dims=None
SHAPES = [
    (3, 1, 1, [1], False),
    (5, 7, 4, [4, 3, 2], False),                # P = 43: rows that are not 16-byte aligned
    (2, 5, 5, [7, 64, 1], False),
    (4, 50, 16, [16, 16], False),
    (3, 9, 64, [64, 64], False),
    (3, 6, 4, [4] * 8, True),
    (6, None, 8, [8, 4], False),
    (3, C16 - 1, 16, [16, 16], False),
    (3, C16, 16, [16, 16], False),
    (3, C16 + 1, 16, [16, 16], False),
    (3, 3 * C16 + 1, 16, [16, 16], False),
]
# use_bias, use_res_net (where the dims allow), last-layer activation, activation, combiner, mask, gradients asked for
OPTIONS = [
    (True, False, False, 'tanh', 'sum', True, 'xp'),
    (False, True, True, 'relu', 'max', True, 'xp'),
    (True, True, False, 'sigmoid', None, True, 'x'),
    (True, False, True, None, 'mean', False, 'p'),
    (False, False, False, torch.tanh, 'min', True, 'xp'),
    (True, False, True, 'relu', _first_half, True, 'xp'),
    (True, True, True, 'tanh', 'min', False, 'x'),
    (False, False, False, 'sigmoid', 'max', False, 'p'),
    (True, False, False, 'linear', None, False, 'xp'),
    (False, True, False, 'tanh', 'mean', True, 'xp'),
    (True, False, True, 'sigmoid', 'sum', True, 'xp'),
    (False, False, True, 'relu', None, True, 'p'),
]
SWEEP = [(si, oi) for si in range(len(SHAPES)) for oi in range(len(OPTIONS)) if (si + oi) % 3 == 0]


def test_sweep_covers_every_option():
    for col in range(7):
        for v in set(o[col] for o in OPTIONS):
            shapes = [SHAPES[si] for si, oi in SWEEP if OPTIONS[oi][col] == v]
            assert shapes, (col, v)
    assert any(OPTIONS[oi][1] and all(d == SHAPES[si][2] for d in SHAPES[si][3]) for si, oi in SWEEP)


@pytest.mark.parametrize('si,oi', SWEEP)
def test_fwd_bwd_vs_oracle(dev, si, oi):
    B, L, D0, dims, auto = SHAPES[si]
    use_bias, res, last_act, act, comb, mask, grads = OPTIONS[oi]
    res = res and all(d == D0 for d in dims)
    gen = torch.Generator().manual_seed(1000 * si + oi)
    x64, p64 = _draw(gen, B, L or 1, D0, dims, use_bias)
    if L is None:
        x64 = x64[:, 0]
    kw = dict(activation=act, use_bias=use_bias, use_res_net=res, output_layer_use_activation=last_act, output_combiner=comb,
              mask_all_zero_embedding=mask)
    x = x64.float().to(dev).requires_grad_('x' in grads)
    p = p64.float().to(dev).requires_grad_('p' in grads)
    y = _layer(dnn_dims=None if auto else dims, **kw)(x, p)
    xr, pr = x64.clone().requires_grad_('x' in grads), p64.clone().requires_grad_('p' in grads)
    ref = C.can_layer(xr, pr, dims, **kw)
    close(y, ref, what='y')
    gy = torch.randn(ref.shape, generator=gen, dtype=torch.float64)
    y.backward(gy.float().to(dev))
    ref.backward(gy)
    if 'x' in grads:
        close(x.grad, xr.grad, what='dx')
    else:
        assert x.grad is None
    if 'p' in grads:
        close(p.grad, pr.grad, what='dparams')
    else:
        assert p.grad is None


def test_empty_batch_and_empty_sequence(dev):
    layer = _layer(dnn_dims=[4, 2])
    assert layer(torch.zeros(0, 3, 4, device=dev), torch.zeros(0, 30, device=dev)).shape == (0, 2)
    none = _layer(dnn_dims=[4, 2], output_combiner=None)
    p = torch.ones(2, 30, device=dev, requires_grad=True)
    out = none(torch.zeros(2, 0, 4, device=dev), p)
    assert out.shape == (2, 0, 2)
    out.sum().backward()
    assert torch.equal(p.grad, torch.zeros_like(p))
    with pytest.raises(ValueError, match='empty axis'):
        layer(torch.zeros(2, 0, 4, device=dev), p)


# ---- ties, determinism, graph capture, memory ------------------------------------------------------------------------
@pytest.mark.parametrize('comb', ['max', 'min'])
def test_ties_share_the_gradient(dev, comb):
    B, L, D0, dims = 2, 3, 16, [16, 16]
    gen = torch.Generator().manual_seed(7)
    x64, p64 = _draw(gen, B, L, D0, dims, True, special=False)
    x64[:, 1] = x64[:, 0]                       # two identical non-zero rows per sample
    x64[0, 2] = x64[0, 0]                       # sample 0: all three rows tie in every column
    x64[1, 2] = 0.0                             # sample 1: a masked row, whose 0 takes part in the extremum
    kw = dict(activation='tanh', output_layer_use_activation=False)
    x, p = x64.float().to(dev).requires_grad_(True), p64.float().to(dev).requires_grad_(True)
    rows = _layer(dnn_dims=dims, output_combiner=None, **kw)(x, p)
    assert torch.equal(rows[:, 0], rows[:, 1]) and torch.equal(rows[0, 0], rows[0, 2])
    y = _layer(dnn_dims=dims, output_combiner=comb, **kw)(x, p)
    xr, pr = x64.clone().requires_grad_(True), p64.clone().requires_grad_(True)
    ref = C.can_layer(xr, pr, dims, output_combiner=comb, **kw)
    close(y, ref, what='y')
    gy = torch.randn(ref.shape, generator=gen, dtype=torch.float64)
    y.backward(gy.float().to(dev))
    ref.backward(gy)
    close(x.grad, xr.grad, what='dx')
    close(p.grad, pr.grad, what='dparams')
    assert torch.equal(x.grad[:, 0], x.grad[:, 1])


def _fwd_bwd(layer, x, p, gy):
    xi, pi = x.clone().requires_grad_(True), p.clone().requires_grad_(True)
    y = layer(xi, pi)
    dx, dp = torch.autograd.grad(y, (xi, pi), gy)
    return y, dx, dp


@pytest.mark.parametrize('comb', ['sum', 'max'])
def test_runs_are_bit_identical(dev, comb):
    B, L, D0, dims = 64, 50, 16, [16, 16]
    gen = torch.Generator().manual_seed(5)
    x64, p64 = _draw(gen, B, L, D0, dims, True)
    x, p = x64.float().to(dev), p64.float().to(dev)
    gy = torch.randn(B, 16, generator=gen).to(dev)
    layer = _layer(dnn_dims=dims, output_combiner=comb)
    a, b = _fwd_bwd(layer, x, p, gy), _fwd_bwd(layer, x, p, gy)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_captured_graph_replays_bit_for_bit(dev):
    B, L, D0, dims = 32, 20, 16, [16, 16]
    gen = torch.Generator().manual_seed(6)
    draw = lambda: [t.float() for t in _draw(gen, B, L, D0, dims, True)]      # noqa: E731
    tx, tp = (t.to(dev).requires_grad_(True) for t in draw())
    gy = torch.randn(B, 16, generator=gen).to(dev)
    layer = _layer(dnn_dims=dims, output_combiner='mean')

    def step():
        y = layer(tx, tp)
        return (y,) + torch.autograd.grad(y, (tx, tp), gy)
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        x, p = draw()                                # new contents, same storage
        with torch.no_grad():
            tx.copy_(x.to(dev))
            tp.copy_(p.to(dev))
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        want = step()
        torch.cuda.synchronize()
        for u, v in zip(got, want):
            assert torch.equal(u, v)
        close(got[0], C.can_layer(x.double(), p.double(), dims, output_combiner='mean'), what='replayed y')


def test_forward_allocates_nothing_proportional_to_b_times_l(dev):
    B, L, D0, dims = 4096, 50, 16, [16, 16]
    x = torch.randn(B, L, D0, device=dev, requires_grad=True)
    p = (torch.randn(B, C.param_size(D0, dims), device=dev) * 0.25).requires_grad_(True)
    layer = _layer(dnn_dims=dims, output_combiner='sum')
    layer(x[:2], p[:2])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = layer(x, p)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert y.numel() * 4 == 256 * 1024
    assert rise <= 256 * 1024 + 2 ** 20, 'forward allocated %.2f MiB above its inputs' % (rise / 2 ** 20)
    assert B * L * 16 * 4 == 12.5 * 2 ** 20                      # one (B, L, D) intermediate of the reference alone
    del y
