"""GPU: BilinearInteractionLayer (csrc/bilinear.hip) against the fp64 oracle of tests/_bilinear_oracle.py, on every route.

Bound: the project's 1e-5.  `out` and every field's dX are held per row (error <= 1e-5 of that row's largest fp64 magnitude), dW against the
tensor's largest magnitude.  Inputs: unit-variance rows, W of std 1/sqrt(D), unit-variance upstream gradient; on these the plain fp32 torch
composition on the CPU stays within 1.7e-6 on the row-wise measure, so the bound leaves about 6x headroom.  Every comparison prints its worst
fraction of the bound; the largest per tensor are printed once more by the last test of the file."""
import os
import re

import numpy as np
import pytest
import torch

import _bilinear_oracle as O

pytestmark = pytest.mark.gpu
RTOL = 1e-5
KINDS = {'all': 0, 'each': 1, 'interaction': 2}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (B, F, D): P = 1; D % 4 != 0; ..; crosses a 16-field block; ..; the D limit; ..; ..; the F limit (P = 2016); ..; one sample; and a shape whose
# F-1 'each' matrices neither fit LDS nor allow 16-byte accesses
SHAPES = [(3, 2, 4), (5, 3, 5), (37, 8, 16), (130, 17, 8), (67, 24, 16), (33, 6, 64), (300, 5, 32), (260, 33, 12), (9, 64, 4), (70, 3, 20),
          (1, 7, 16), (2, 40, 63)]
WORST = {}


def _consts():
    src = open(os.path.join(ROOT, 'rec_now_amd', 'csrc', 'bilinear.hip')).read()
    return {k: int(v) for k, v in re.findall(r'#define (BIL_[A-Z_]+) \(?(\d+)\)?\s', src)}


def _multi_tile_batch(F, D):
    """A batch at which, at (F, D), some workgroup of every route takes more than one row tile (or sample) and the last tile is ragged: more
    tiles than the largest fixed grid at the largest tile either TILE kernel uses, plus one tile and a part of one."""
    c = _consts()
    dp = (D + 3) // 4 * 4
    lanes = 1
    while lanes < dp // 4:
        lanes *= 2
    r_fwd = max(1, min(c['BIL_TILE_MAX_ROWS'], c['BIL_TILE_X_FLOATS'] // (F * dp)))
    r_bwd = max(1, min(256 // lanes, c['BIL_TILE_DX_FLOATS'] // (F * dp)))
    grid = max(c['BIL_TILE_GRID'], c['BIL_ROW_GRID'])
    return grid * max(r_fwd, r_bwd, 4) + max(r_fwd, r_bwd) + 37


def _layer(kind, W, dev, F, trainable=True):
    from rec_now_amd.layers.bilinear_interaction_layer import BilinearInteractionLayer
    lay = BilinearInteractionLayer(kind, trainable=trainable)
    lay._build_device = dev
    lay.build([(1, W.shape[1])] * F)
    lay.set_weights_by_name({'bilinear_weight': W})
    return lay


def _run(lay, xs, g):
    """One forward + backward.  Returns (out, [dX_f], dW or None) as device tensors."""
    leaves = [x.detach().requires_grad_(True) for x in xs]
    out = lay(leaves)
    wanted = leaves + ([lay.bilinear_weight] if lay.bilinear_weight.requires_grad else [])
    grads = torch.autograd.grad(out, wanted, g)
    return out.detach(), list(grads[:len(xs)]), (grads[len(xs)] if len(grads) > len(xs) else None)


def _hold(what, got, ref, measure, key):
    frac = measure(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, ref) / RTOL
    print('%s %s: %.3f of the bound' % (key, what, frac))
    WORST[what] = max(WORST.get(what, 0.0), frac)
    assert frac <= 1.0, '%s of %s: %.3g of the 1e-5 bound' % (what, key, frac)


def _check(dev, xs, W, g, kind, key, transform=None):
    """Runs the layer on (xs, W, g) (float32 numpy) and holds out, every dX and dW to the fp64 oracle."""
    lay = _layer(kind, W, dev, len(xs))
    txs = [torch.from_numpy(x).to(dev) for x in xs]
    if transform is not None:
        txs = transform(txs)
    out, dxs, dW = _run(lay, txs, torch.from_numpy(g).to(dev))
    ref = O.forward(xs, W, kind)
    rdx, rdw = O.backward(xs, W, kind, g)
    assert out.shape == ref.shape and out.dtype == torch.float32
    _hold('out', out, ref, O.relrow, key)
    for f in range(len(xs)):
        _hold('dX', dxs[f], rdx[f], O.relrow, key)
    _hold('dW', dW, rdw, O.reltensor, key)
    return out, dxs, dW


@pytest.mark.parametrize('kind', O.TYPES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'B%d-F%d-D%d' % s)
def test_matches_the_oracle(dev, shape, kind):
    B, F, D = shape
    xs, W, g = O.draw(np.random.default_rng(B * 1000 + F * 10 + D), B, F, D, kind)
    _check(dev, xs, W, g, kind, '%s %s' % (shape, kind))


@pytest.mark.parametrize('kind', O.TYPES)
def test_more_tiles_than_workgroups_and_a_ragged_last_tile(dev, kind):
    F, D = 3, 4
    B = _multi_tile_batch(F, D)
    c = _consts()
    assert B > c['BIL_TILE_GRID'] * 256 and B % 256 != 0 and B % 64 != 0 and B > 4 * c['BIL_ROW_GRID']
    xs, W, g = O.draw(np.random.default_rng(11), B, F, D, kind)
    _check(dev, xs, W, g, kind, '(%d, %d, %d) %s' % (B, F, D, kind))


def test_every_route_is_reached(dev):
    """Every (kernel family, access width) pair the dispatcher and the kernels can pick, in both directions, is reached by a case of
    test_matches_the_oracle: ROW with the weights in LDS / read through L2, TILE; 16-byte accesses (D % 4 == 0) and guarded 4-byte ones."""
    from rec_now_amd import _lib
    lib = _lib.load()
    seen = set()
    for (B, F, D) in SHAPES:
        for kind, code in KINDS.items():
            for bwd in (0, 1):
                seen.add((lib.recnow_bilinear_route(F, D, code, bwd), D % 4 == 0, bwd))
    assert seen == {(r, v, b) for r in (0, 1, 2) for v in (False, True) for b in (0, 1)}
    # the ROW backward with one wave per workgroup (its three tiles of 64 x 64 leave no room for more), and the weight-gradient partials with
    # one and with several row chunks
    assert lib.recnow_bilinear_route(64, 64, 0, 1) == 1 and lib.recnow_bilinear_route(6, 64, 0, 0) == 0
    assert any(B > _consts()['BIL_DW_ROWS'] for B, _, _ in SHAPES) and any(B <= _consts()['BIL_DW_ROWS'] for B, _, _ in SHAPES)


@pytest.mark.parametrize('kind', O.TYPES)
def test_empty_batch_and_single_field(dev, kind):
    from rec_now_amd.layers.bilinear_interaction_layer import BilinearInteractionLayer
    lay = BilinearInteractionLayer(kind)
    xs = [torch.zeros(0, 8, device=dev, requires_grad=True) for _ in range(4)]
    out = lay(xs)
    assert tuple(out.shape) == (0, 6 * 8)
    grads = torch.autograd.grad(out, xs + [lay.bilinear_weight], torch.zeros_like(out))
    assert all(tuple(a.shape) == (0, 8) for a in grads[:4]) and float(grads[4].abs().max()) == 0.0
    one = BilinearInteractionLayer(kind)
    x = torch.randn(5, 8, device=dev, requires_grad=True)
    out = one([x])
    assert tuple(out.shape) == (5, 0) and tuple(one.bilinear_weight.shape) == (1, 8, 8)
    gx, gw = torch.autograd.grad(out, [x, one.bilinear_weight], torch.zeros_like(out))
    assert float(gx.abs().max()) == 0.0 and float(gw.abs().max()) == 0.0


@pytest.mark.parametrize('kind', O.TYPES)
def test_column_views_and_rows_aligned_to_four_bytes_only(dev, kind):
    B, F, D = 41, 6, 8
    xs, W, g = O.draw(np.random.default_rng(21), B, F, D, kind)

    def views(txs):                                    # the fields as column views of one (B, F*D) tensor
        cat = torch.cat(txs, 1)
        return [cat[:, f * D:(f + 1) * D] for f in range(F)]

    def offset(txs):                                   # contiguous fields whose storage starts one float into an allocation
        out = []
        for t in txs:
            buf = torch.empty(t.numel() + 1, device=dev)
            buf[1:].copy_(t.reshape(-1))
            v = buf[1:].view(B, D)
            assert v.is_contiguous() and v.data_ptr() % 16 == 4
            out.append(v)
        return out
    a = _check(dev, xs, W, g, kind, 'views %s' % kind, views)
    b = _check(dev, xs, W, g, kind, 'offset %s' % kind, offset)
    c = _check(dev, xs, W, g, kind, 'plain %s' % kind)
    for got in (a, b):                                 # the access width changes no arithmetic
        assert torch.equal(got[0], c[0]) and torch.equal(got[2], c[2]) and all(torch.equal(p, q) for p, q in zip(got[1], c[1]))


@pytest.mark.parametrize('kind', O.TYPES)
def test_zero_rows_negative_zero_and_zeros_in_the_gradient(dev, kind):
    B, F, D = 19, 5, 12
    xs, W, g = O.draw(np.random.default_rng(31), B, F, D, kind)
    for f in range(F):
        xs[f][3] = 0.0
        xs[f][7] = -0.0
    xs[2][11] = 0.0                                    # one field of a sample only
    g[5] = 0.0
    g[:, ::3] = 0.0
    out, dxs, dW = _check(dev, xs, W, g, kind, 'zeros %s' % kind)
    assert float(out[3].abs().max()) == 0.0 and float(out[7].abs().max()) == 0.0
    assert all(float(d[5].abs().max()) == 0.0 for d in dxs)
    assert all(bool(torch.isfinite(t).all()) for t in [out, dW] + dxs)


@pytest.mark.parametrize('kind', O.TYPES)
def test_a_nan_stays_in_its_sample(dev, kind):
    B, F, D = 70, 6, 16
    xs, W, g = O.draw(np.random.default_rng(41), B, F, D, kind)
    lay = _layer(kind, W, dev, F)
    tg = torch.from_numpy(g).to(dev)
    clean = _run(lay, [torch.from_numpy(x).to(dev) for x in xs], tg)
    xs[2][33, 5] = np.nan
    dirty = _run(lay, [torch.from_numpy(x).to(dev) for x in xs], tg)
    keep = torch.ones(B, dtype=torch.bool, device=dev)
    keep[33] = False
    assert torch.equal(dirty[0][keep], clean[0][keep]) and bool(torch.isnan(dirty[0][33]).any())
    for f in range(F):
        assert torch.equal(dirty[1][f][keep], clean[1][f][keep])
    assert bool(torch.isnan(torch.stack(dirty[1])[:, 33]).any())


@pytest.mark.parametrize('kind', O.TYPES)
def test_frozen_weight_skips_dw_and_runs_repeat_bit_for_bit(dev, kind):
    B, F, D = 300, 9, 16
    xs, W, g = O.draw(np.random.default_rng(51), B, F, D, kind)
    txs, tg = [torch.from_numpy(x).to(dev) for x in xs], torch.from_numpy(g).to(dev)
    lay = _layer(kind, W, dev, F)
    first, second = _run(lay, txs, tg), _run(lay, txs, tg)
    assert torch.equal(first[0], second[0]) and torch.equal(first[2], second[2])
    assert all(torch.equal(p, q) for p, q in zip(first[1], second[1]))
    frozen = _run(_layer(kind, W, dev, F, trainable=False), txs, tg)
    assert frozen[2] is None
    assert torch.equal(frozen[0], first[0]) and all(torch.equal(p, q) for p, q in zip(frozen[1], first[1]))


@pytest.mark.parametrize('kind', O.TYPES)
def test_graph_capture_replays_bit_for_bit(dev, kind):
    B, F, D = 129, 7, 16
    rng = np.random.default_rng(61)
    xs, W, g = O.draw(rng, B, F, D, kind)
    lay = _layer(kind, W, dev, F)
    txs = [torch.from_numpy(x).to(dev).requires_grad_(True) for x in xs]
    tg = torch.from_numpy(g).to(dev)

    def step():
        out = lay(txs)
        return (out,) + torch.autograd.grad(out, txs + [lay.bilinear_weight], tg)
    step()                                             # the pointer tables of the inputs are uploaded (and cached) outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        new, _, ng = O.draw(rng, B, F, D, kind)        # new contents, same storage
        with torch.no_grad():
            for t, x in zip(txs, new):
                t.copy_(torch.from_numpy(x))
            tg.copy_(torch.from_numpy(ng))
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        assert all(torch.equal(a, b) for a, b in zip(outs, eager))


def test_forward_allocates_only_its_output(dev):
    B, F, D = 4096, 8, 16
    xs = [torch.randn(B, D, device=dev) for _ in range(F)]
    for kind in O.TYPES:
        from rec_now_amd.layers.bilinear_interaction_layer import BilinearInteractionLayer
        lay = BilinearInteractionLayer(kind)
        with torch.no_grad():
            lay([x[:2] for x in xs])
            lay(xs)                                    # the pointer table of this call is uploaded once per content
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            y = lay(xs)
            torch.cuda.synchronize()
            rise = torch.cuda.max_memory_allocated() - base
        assert y.numel() * 4 == 28 * 16 * 4096 * 4
        assert rise <= y.numel() * 4 + 2 ** 20, '%s forward allocated %.2f MiB above its inputs' % (kind, rise / 2 ** 20)
        del y


def test_senet_bilinear_dense_module_matches_fp64_autograd(dev):
    """SENETLayer -> BilinearInteractionLayer -> MultiDenseLayer head: every parameter gradient against fp64 autograd of the oracles."""
    import dense_ref as R
    from rec_now_amd.layers.bilinear_interaction_layer import BilinearInteractionLayer
    from rec_now_amd.layers.multi_dense_layer import MultiDenseLayer
    from rec_now_amd.layers.senet_layer import SENETLayer
    torch.manual_seed(5)
    B, F, D = 96, 6, 8
    rng = np.random.default_rng(71)
    xs = [rng.standard_normal((B, D)).astype(np.float32) for _ in range(F)]
    senet, cross, head = SENETLayer(0.5), BilinearInteractionLayer('interaction'), MultiDenseLayer(4, 1)
    txs = [torch.from_numpy(x).to(dev) for x in xs]
    gy = torch.from_numpy(rng.standard_normal((B, 4)).astype(np.float32)).to(dev)

    def model(fields):
        s = senet(fields)
        return head(cross([s[:, f * D:(f + 1) * D] for f in range(F)])).reshape(B, 4)
    y = model(txs)
    params = {'senet0/kernel': senet.senet[0].kernel, 'senet0/bias': senet.senet[0].bias, 'senet1/kernel': senet.senet[1].kernel,
              'senet1/bias': senet.senet[1].bias, 'bilinear_weight': cross.bilinear_weight, 'head/kernel': head.kernel, 'head/bias': head.bias}
    grads = torch.autograd.grad(y, list(params.values()), gy)
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in params.items()}
    x64 = [torch.from_numpy(x).double() for x in xs]
    s = R.senet_layer(x64, [p64['senet0/kernel'], p64['senet1/kernel']], [p64['senet0/bias'], p64['senet1/bias']])
    ii, jj = torch.triu_indices(F, F, 1)
    X = s.reshape(B, F, D)
    z = (torch.einsum('bpk,pkd->bpd', X[:, ii], p64['bilinear_weight']) * X[:, jj]).reshape(B, -1)
    y64 = R.multi_dense_layer(z, p64['head/kernel'], p64['head/bias']).reshape(B, 4)
    _hold('module out', y, y64.detach().numpy(), O.reltensor, 'module')
    g64 = torch.autograd.grad(y64, list(p64.values()), gy.cpu().double())
    for name, got, want in zip(params, grads, g64):
        _hold('module d ' + name, got, want.numpy(), O.reltensor, 'module')


def test_zz_report_the_worst_fractions():
    """Last in the file: the largest fraction of the 1e-5 bound seen per tensor by the tests above (printed; the bound itself is asserted there)."""
    for what in sorted(WORST):
        print('worst %-24s %.3f of the bound' % (what, WORST[what]))
    assert all(v <= 1.0 for v in WORST.values())
