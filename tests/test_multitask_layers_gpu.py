"""MMOELayer and PLELayer against the fp64 oracle (oracle/dense_ref.mmoe_layer / ple_layer) with EVERY gradient: every task output, dx and
every entry of named_weights().  Input rows are scaled by 2^-k (k = 0..8); outputs and dx are held per row to 1e-5 x the row's max |ref|, weight
gradients per expert slice and column to 1e-5 x the column's max |ref| (bias gradients, whose columns have one entry: REL_DB below), and every
tensor to the norm bound of the layer tests; the worst margins are printed.
The oracle's `layers` structure comes from the built layer itself (tests/_ple_oracle.py), which is first held to the golden fixture."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, 'oracle')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dense_ref as R                      # noqa: E402
import _ple_oracle as P                    # noqa: E402
from _chunked_oracle import close          # noqa: E402

pytestmark = pytest.mark.gpu
REL = 1e-5
# Bias gradients, per entry: a "column" of a bias (N, 1, U) or (units,) is ONE number, a sum over the batch whose terms change sign, so its own
# magnitude is no scale for its error.  The same layers in plain fp32 on the CPU (the layer classes with their two ops replaced by torch fp32
# matmul / softmax, same data) reach, as their worst bias entry per configuration below, 6.6 / 265.5 / 0.04 / 96.8 / 6.4 / 20.4 x REL (MMoE) and
# 4.7 / 18.0 / 0.38 / 7.0 / 8.5 x REL (PLE), against 0.62 x REL for the worst kernel column and 0.25 x REL for the worst row: the entries in
# question are sums that cancel to 1e-4 of their terms.  Twice the worst of the restatement; the kernels measured 1.6 - 178 x REL on the same
# entries.  Every bias gradient is also held to the norm bound (1e-5 x the tensor's max) like every other tensor.
REL_DB = 2 * 265.5 * REL

GOLDEN_PLE = (2, [[2, 3], [2, 3], [3, 2]], [4, 3, 2], 1)


def _random_weights(layer, rng, lim=0.2):
    layer.set_weights_by_name({k: rng.uniform(-lim, lim, tuple(v.shape)).astype(np.float32) for k, v in layer.named_weights().items()})


def _margins(what, outs, routs, dx, rdx, layer, by_key):
    """{tensor: worst fraction of its bound} of every output, dx and every weight gradient (after the norm bound of each), printed"""
    m = {}
    for t, (o, ro) in enumerate(zip(outs, routs)):
        close(o, ro, what='%s out %d' % (what, t))
        m['out %d' % t] = P.row_margin(P.torch_np(ro), P.torch_np(o), REL)
    close(dx, rdx, what='%s dx' % what)
    m['dx'] = P.row_margin(P.torch_np(rdx), P.torch_np(dx), REL)
    weights = layer.named_weights()
    assert set(by_key) == set(weights)
    for k, p in weights.items():
        assert p.grad is not None and by_key[k].grad is not None, '%s: no gradient for %s' % (what, k)
        close(p.grad, by_key[k].grad, what='%s d %s' % (what, k))
        m['d ' + k] = P.column_margin(P.torch_np(by_key[k].grad), P.torch_np(p.grad), REL_DB if k.endswith('/bias') else REL)
    wo = max((k for k in m if not k.startswith('d ')), key=m.get)
    wk = max((k for k in m if k.startswith('d ') and not k.endswith('/bias')), key=m.get)
    wb = max((k for k in m if k.endswith('/bias')), key=m.get)
    print('%s: worst margins as fractions of the bound: per row %.3f (%s); per column of the kernel gradients %.3f (%s); per entry of the bias '
          'gradients %.3f (%s); %d weight gradients' % (what, m[wo], wo, m[wk], wk, m[wb], wb, len(weights)))
    return m


def _compare(*args):
    m = _margins(*args)
    over = {k: v for k, v in m.items() if not v <= 1.0}
    assert not over, '%s: beyond the per-row / per-column bound (fraction of it): %r' % (args[0], over)


# ---- the helper against the golden fixture ---------------------------------------------------------------------------------------------------------
def test_oracle_layers_equals_the_fixture_structure(dev, golden):
    from rec_now_amd.layers.ple_layer import PLELayer
    from test_layers_gpu import _load_ple
    from test_oracle_golden import ple_layers_from_fixture
    g = golden('ple')
    layer = PLELayer(*GOLDEN_PLE, name='PLE')
    layer(torch.from_numpy(g['inputs']).to(dev))
    _load_ple(layer, g)
    got, by_key = P.oracle_layers(layer, to=lambda p: p.detach().cpu().numpy())
    want = ple_layers_from_fixture(g, to=lambda v: np.asarray(v))
    assert len(got) == len(want) == 3
    n = 0
    for lg, lw in zip(got, want):
        assert len(lg['dnn']) == len(lw['dnn']) and len(lg['gate']) == len(lw['gate'])
        for sg, sw in zip(lg['dnn'], lw['dnn']):
            assert len(sg) == len(sw)
            for (kg, bg), (kw, bw) in zip(sg, sw):
                assert np.array_equal(kg, kw.reshape(kg.shape)) and np.array_equal(bg, bw.reshape(bg.shape))
                n += 2
        for gg, gw in zip(lg['gate'], lw['gate']):
            assert (gg is None) == (gw is None)
            if gg is not None:
                assert np.array_equal(gg[0], gw[0].reshape(gg[0].shape)) and np.array_equal(gg[1], gw[1].reshape(gg[1].shape))
                n += 2
    assert n == len(by_key) == len(layer.named_weights())


# ---- MMoE --------------------------------------------------------------------------------------------------------------------------------------
MMOE = [(700, 96, 3, 5, [64, 32], 'tanh'), (700, 96, 3, 5, [64, 32], None), (300, 40, 1, 1, [8], 'tanh'), (257, 64, 2, 64, [16], 'tanh'),
        (4133, 64, 2, 4, [64, 130], 'tanh'), (4133, 64, 2, 4, [64, 130], None)]


@pytest.mark.parametrize('B,D,T,N,dims,act', MMOE, ids=['b%d_d%d_t%d_n%d_%s_%s' % (c[0], c[1], c[2], c[3], 'x'.join(map(str, c[4])), c[5]) for c in MMOE])
def test_mmoe_every_gradient_vs_oracle(dev, B, D, T, N, dims, act):
    from rec_now_amd.layers.mmoe_layer import MMOELayer
    rng = np.random.default_rng(B + 7 * N + T)
    x = P.scaled_rows(rng, B, D)
    layer = MMOELayer(T, N, dims, activation=act, name='m')
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    layer(xd)
    _random_weights(layer, rng)
    gy = rng.normal(size=(T, B, dims[-1])).astype(np.float32)
    y = layer(xd)
    y.backward(torch.from_numpy(gy).to(dev))
    ks, bs, gk, gb, by_key = P.mmoe_oracle_weights(layer)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    ry = R.mmoe_layer(x64, ks, bs, gk, gb, activation=act)
    ry.backward(torch.from_numpy(gy).double())
    _compare('mmoe', list(y.unbind(0)), list(ry.unbind(0)), xd.grad, x64.grad, layer, by_key)


def test_mmoe_65_experts_raises(dev):
    """One expert more than the mixing kernel takes (64): today the layer raises from recnow_moe_mix_fwd rather than compute something else."""
    from rec_now_amd.layers.mmoe_layer import MMOELayer
    layer = MMOELayer(2, 65, [8], name='m')
    x = torch.from_numpy(P.scaled_rows(np.random.default_rng(65), 33, 16)).to(dev)
    with pytest.raises(RuntimeError, match='RECNOW_EUNSUPPORTED'):
        layer(x)


# ---- PLE ---------------------------------------------------------------------------------------------------------------------------------------
CONFIG5_SMALL = (3, [[64, 32], [32, 16]], 2, 1)
PLE = [
    ('golden', GOLDEN_PLE, 333, 4, 'tanh'),
    ('config5_small', CONFIG5_SMALL, 700, 96, 'tanh'),            # expert stacks N = 2, U >= 64: the batched bias sums
    ('ragged_two_shared', (2, [[16], [8]], [[1, 2, 3, 1], [2, 1, 1, 2]], 2), 300, 24, None),
    ('single_layer', (2, [[16, 8]], 2, 1), 300, 24, 'tanh'),      # the shared group has no gate at all
    ('config5_small_narrow', CONFIG5_SMALL, 4096 + 37, 64, 'tanh'),      # gate Dense layers (N = 1) on k_narrow_dense and k_small_xty
]


@pytest.mark.parametrize('name,args,B,D,act', PLE, ids=[c[0] for c in PLE])
def test_ple_every_gradient_vs_oracle(dev, golden, name, args, B, D, act):
    from rec_now_amd.layers.ple_layer import PLELayer
    rng = np.random.default_rng(B + D)
    x = P.scaled_rows(rng, B, D)
    layer = PLELayer(*args, name='PLE', activation=act)
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    layer(xd)
    if name == 'golden':
        from test_layers_gpu import _load_ple
        _load_ple(layer, golden('ple'))
    else:
        _random_weights(layer, rng)
    outs = layer(xd)
    assert len(outs) == args[0]
    gys = [rng.normal(size=tuple(o.shape)).astype(np.float32) for o in outs]
    sum((o * torch.from_numpy(gy).to(dev)).sum() for o, gy in zip(outs, gys)).backward()
    layers, by_key = P.oracle_layers(layer)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    routs = R.ple_layer(x64, layers, layer.is_shared_tasks, activation=act)
    sum((o * torch.from_numpy(gy).double()).sum() for o, gy in zip(routs, gys)).backward()
    if name == 'single_layer':
        assert layer.gates[0][0] is None
    _compare('ple ' + name, outs, routs, xd.grad, x64.grad, layer, by_key)
