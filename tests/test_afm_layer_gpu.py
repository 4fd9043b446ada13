"""GPU: AFMLayer (csrc/afm.hip) against the fp64 oracle of tests/_afm_oracle.py, on every access width and both directions.

Bound: the project's 1e-5.  The pooled vector v (projection=False) is held per row (error <= 1e-5 of that row's largest fp64 magnitude); the
projected output against sum_c |v_c p_c| of its sample (the dot product may cancel; the oracle returns that scale); every field's dX per row (a
row is one field of one sample); each of dW, db, dh, dp against its tensor's largest magnitude.  Inputs: _afm_oracle.draw -- unit-variance X, W of
std 1/sqrt(D), b of std 0.1, h and p of std 1/sqrt(A) and 1/sqrt(D), a unit-variance upstream gradient; samples with a hidden value within 1e-5
of a ReLU gate are redrawn, so no entry is left out of any comparison.
On the shapes of test_matches_the_oracle the plain fp32 torch composition on the CPU stays within 0.021 (out), 0.042 (v), 0.176 (dX), 0.042 (dW),
0.096 (db), 0.157 (dh) and 0.043 (dp) of the bound on these measures ((2, 64, 64, 64): 0.004 out, 0.164 dX, 0.027 dW, 0.075 dh), so the bound leaves
more than 5x headroom over plain fp32.  Two exceptions, neither met by widening the bound.  (1) An fp32 score of magnitude 100 carries an absolute
error of about 1e-5, which the exponential turns into a relative error of the attention weights: the two large-score tests use exactly representable
inputs (their docstrings give the composition's figures on random ones).  (2) db_a = h_a sum_k de_k [z_ka > 0] of a unit whose gate is open for
every pair is exactly 0 (the softmax gradient sums to 0), so its fp64 value is rounding noise and a per-tensor ratio means nothing: where every open
gate is always open ((2, 64, 64, 64), whose gates the bias fixes, and units 0 .. 2 of the overflow test) db is held against the largest
sum_k |dz_ka| instead, as the projected output is against sum_c |v_c p_c|.
Every comparison prints its fraction of the bound; the largest per tensor are printed once more by the last test of the file."""
import os
import re

import numpy as np
import pytest
import torch

import _afm_oracle as O

pytestmark = pytest.mark.gpu
RTOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (B, F, D, A): F = 2; nothing divisible by 4; more fields than a 16-lane group; the benchmark shape; the F limit, P = 2016; the D and A limits;
# B = 1 and A = 1; all limits at once (its gates are fixed by the bias, see _limits_case); and D % 4 != 0 beside A % 4 == 0
SHAPES = [(3, 2, 4, 4), (5, 5, 3, 3), (37, 17, 8, 5), (67, 24, 16, 16), (9, 64, 4, 4), (6, 12, 64, 64), (1, 7, 16, 1), (2, 64, 64, 64), (4, 6, 6, 8)]
CASES = [(s, proj) for s in SHAPES[:5] + SHAPES[6:7] + SHAPES[8:] for proj in (True, False)] + [(SHAPES[5], False), (SHAPES[7], True)]
WORST = {}
NAMES = ('attention_W', 'attention_b', 'projection_h', 'projection_p')
GRADS = ('dW', 'db', 'dh', 'dp')
_CASES = {}


def _consts():
    src = open(os.path.join(ROOT, 'rec_now_amd', 'csrc', 'afm.hip')).read()
    return {k: int(v) for k, v in re.findall(r'#define (AFM_[A-Z_]+) \(?(\d+)\)?\s', src)}


def _freeze(case):
    for a in [case['X'], case['g']] + [w for w in case['W'] if w is not None]:
        a.setflags(write=False)
    return case


def _case(seed, B, F, D, A, proj=True, h_scale=1.0, edit=None):
    """Inputs and their fp64 results, computed once per distinct case and shared by the tests."""
    key = (seed, B, F, D, A, proj, h_scale, edit)
    if key not in _CASES:
        X, W, b, h, p, g = O.draw(np.random.default_rng(seed), B, F, D, A, proj, h_scale)
        if edit is not None:
            edit(X, g)
        _CASES[key] = _freeze(dict(X=X, W=(W, b, h, p), g=g, ref=O.run(X, W, b, h, p, g)))
    return _CASES[key]


def _limits_case(proj=True):
    """(2, 64, 64, 64): with P A = 129 024 hidden values per sample nearly every random sample has one within 1e-5 of its gate, so the gates are
    fixed by the bias instead of by redraws: half the units get b_a = +1.25 max_k sum_c |W_ca p_c| (always open), half -1.25 that (always shut)."""
    key = ('limits', proj)
    if key not in _CASES:
        rng = np.random.default_rng(2064)
        B, F, D, A = SHAPES[7]
        X = rng.standard_normal((B, F, D)).astype(np.float32)
        W = (rng.standard_normal((D, A)) / 8).astype(np.float32)
        h, p = (rng.standard_normal(A) / 8).astype(np.float32), (rng.standard_normal(D) / 8).astype(np.float32)
        ii, jj = np.triu_indices(F, 1)
        mag = (np.abs(X[:, ii].astype(np.float64) * X[:, jj]) @ np.abs(W.astype(np.float64))).max()
        b = (1.25 * mag * np.where(np.arange(A) % 2 == 0, 1.0, -1.0)).astype(np.float32)
        assert O.gate_margin(X, W, b).min() > 0.1
        g = rng.standard_normal((B, 1 if proj else D)).astype(np.float32)
        p = p if proj else None
        _CASES[key] = _freeze(dict(X=X, W=(W, b, h, p), g=g, ref=O.run(X, W, b, h, p, g)))
    return _CASES[key]


def _layer(case, dev, trainable=True):
    from rec_now_amd.layers.afm_layer import AFMLayer
    W, b, h, p = case['W']
    lay = AFMLayer(W.shape[1], projection=p is not None, trainable=trainable)
    lay._build_device = dev
    lay.build(case['X'].shape)
    lay.set_weights_by_name({n: w.copy() for n, w in zip(NAMES, case['W']) if w is not None})
    return lay


def _weights(lay):
    return [w for w in (lay.attention_W, lay.attention_b, lay.projection_h, lay.projection_p) if w is not None]


def _as_list(x):
    return [x[:, f].contiguous() for f in range(x.shape[1])]


def _run(lay, inputs, g):
    """One forward + backward.  inputs: a (B, F, D) tensor or a list of (B, D).  Returns (out, dX stacked (B, F, D), [dW ..] or None)."""
    three_d = isinstance(inputs, torch.Tensor)
    leaves = [inputs.detach().requires_grad_(True)] if three_d else [x.detach().requires_grad_(True) for x in inputs]
    out = lay(leaves[0] if three_d else leaves)
    ws = [w for w in _weights(lay) if w.requires_grad]
    grads = torch.autograd.grad(out, leaves + ws, g.reshape(out.shape))
    dx = grads[0] if three_d else torch.stack(grads[:len(leaves)], 1)
    return out.detach(), dx, (list(grads[len(leaves):]) if ws else None)


def _hold(what, got, ref, measure, key):
    frac = measure(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, ref) / RTOL
    print('%s %s: %.3f of the bound' % (key, what, frac))
    WORST[what] = max(WORST.get(what, 0.0), frac)
    assert frac <= 1.0, '%s of %s: %.3g of the 1e-5 bound' % (what, key, frac)


def _hold_all(got, case, key, db_cancels=False):
    """db_cancels: every open gate of the case is open for all pairs, so db_a = h_a sum_k de_k = 0 cancels exactly; like the projected output,
    db is then held against the sum of the magnitudes of its terms (the oracle's db_abs)."""
    ref = case['ref']
    B, F, D = case['X'].shape
    proj = case['W'][3] is not None
    assert got[0].dtype == torch.float32 and tuple(got[0].shape) == ((B, 1) if proj else (B, D))
    if proj:
        _hold('out', got[0], ref['out'], lambda a, r: O.relscale(a, r, ref['scale']), key)
    else:
        _hold('v', got[0], ref['out'], O.relrow, key)
    _hold('dX', got[1].reshape(B * F, D), ref['dX'].reshape(B * F, D), O.relrow, key)
    for name, dw in zip(GRADS, got[2]):
        if name == 'db' and db_cancels:
            _hold('db (cancelling)', dw, ref['db'], lambda a, r: O.relscale(a.reshape(1, -1), r.reshape(1, -1), ref['db_abs'].max()), key)
        else:
            _hold(name, dw, ref[name], O.reltensor, key)


def _check(dev, case, key, three_d=False, db_cancels=False):
    """Runs the layer on the case and holds the output, every field's dX and every weight gradient to the fp64 oracle."""
    x = torch.tensor(case['X']).to(dev)
    got = _run(_layer(case, dev), x if three_d else _as_list(x), torch.tensor(case['g']).to(dev))
    _hold_all(got, case, key, db_cancels)
    return got


def _same(a, b):
    return torch.equal(a[0].reshape(-1), b[0].reshape(-1)) and torch.equal(a[1], b[1]) and (
        (a[2] is None and b[2] is None) or all(torch.equal(p, q) for p, q in zip(a[2], b[2])))


@pytest.mark.parametrize('shape,proj', CASES, ids=lambda s: ('B%d-F%d-D%d-A%d' % s) if isinstance(s, tuple) else ('proj' if s else 'pooled'))
def test_matches_the_oracle(dev, shape, proj):
    B, F, D, A = shape
    case = _limits_case(proj) if shape == SHAPES[7] else _case(B * 1000 + F * 10 + D, B, F, D, A, proj)
    got = _check(dev, case, '%s %s' % (shape, 'proj' if proj else 'pooled'), three_d=(F % 2 == 1), db_cancels=(shape == SHAPES[7]))
    if F == 2:                                             # a = 1: nothing reaches the attention network
        assert all(float(w.abs().max()) == 0.0 for w in got[2][:3])


def test_more_samples_than_waves_and_a_ragged_last_chunk(dev):
    """More samples than AFM_MAXG waves of AFM_DW_ROWS samples: every wave walks a chunk of several samples, and the last wave's chunk is short."""
    c = _consts()
    B = c['AFM_MAXG'] * c['AFM_DW_ROWS'] + 2 * c['AFM_MAXG'] + 37
    rows = -(-B // c['AFM_MAXG'])                         # samples per wave
    assert rows > c['AFM_DW_ROWS'] and B % rows != 0 and -(-B // rows) <= c['AFM_MAXG']
    _check(dev, _case(11, B, 3, 4, 4), '(%d, 3, 4, 4)' % B)


def test_every_route_is_reached(dev):
    """Every (route, access width, direction) the dispatcher and the kernels can pick is reached by a case of test_matches_the_oracle: there is
    one route; fields and dX go by 16 bytes with D % 4 == 0 and by guarded 4-byte accesses otherwise, the weights and their partials likewise
    with A % 4 == 0, and both mixed combinations occur; each direction runs on every case."""
    from rec_now_amd import _lib
    lib = _lib.load()
    seen = set()
    for (B, F, D, A), _ in CASES:
        for bwd in (0, 1):
            seen.add((lib.recnow_afm_route(F, D, A, bwd), D % 4 == 0, A % 4 == 0, bwd))
    assert seen == {(0, vd, va, b) for vd in (False, True) for va in (False, True) for b in (0, 1)}
    assert any(B > _consts()['AFM_DW_ROWS'] for (B, _, _, _), _ in CASES) and any(B == 1 for (B, _, _, _), _ in CASES)
    assert any(F > 32 for (_, F, _, _), _ in CASES) and any(F * (F - 1) // 2 < 64 for (_, F, _, _), _ in CASES)


def test_empty_batch_and_a_single_field(dev):
    from rec_now_amd.layers.afm_layer import AFMLayer
    for proj in (True, False):
        lay = AFMLayer(4, projection=proj)
        xs = [torch.zeros(0, 8, device=dev, requires_grad=True) for _ in range(3)]
        out = lay(xs)
        assert tuple(out.shape) == ((0, 1) if proj else (0, 8))
        grads = torch.autograd.grad(out, xs + _weights(lay), torch.zeros_like(out))
        assert all(tuple(a.shape) == (0, 8) for a in grads[:3]) and all(float(a.abs().max()) == 0.0 for a in grads[3:])
        x3 = torch.zeros(0, 3, 8, device=dev, requires_grad=True)
        assert tuple(torch.autograd.grad(lay(x3), [x3], torch.zeros_like(out))[0].shape) == (0, 3, 8)
        one = AFMLayer(4, projection=proj)
        x1 = torch.randn(5, 1, 8, device=dev, requires_grad=True)
        y = one(x1)
        assert tuple(y.shape) == ((5, 1) if proj else (5, 8)) and float(y.detach().abs().max()) == 0.0
        grads = torch.autograd.grad(y, [x1] + _weights(one), torch.ones_like(y))
        assert all(float(a.abs().max()) == 0.0 for a in grads) and tuple(grads[0].shape) == (5, 1, 8)


def test_layouts_agree_bit_for_bit(dev):
    """A list of contiguous fields, a (B, F, D) tensor, column views of a (B, F*D) tensor and storage that starts one float into an allocation
    (4-byte accesses) give the same bits."""
    case = _case(21, 41, 6, 8, 4)
    B, F, D = case['X'].shape
    lay = _layer(case, dev)
    x = torch.tensor(case['X']).to(dev)
    g = torch.tensor(case['g']).to(dev)
    plain = _check(dev, case, 'layouts')
    flat = x.reshape(B, F * D)
    buf = torch.empty(x.numel() + 1, device=dev)
    buf[1:].copy_(x.reshape(-1))
    off = buf[1:].view(B, F, D)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    for other in (x, [flat[:, f * D:(f + 1) * D] for f in range(F)], off, [off[:, f] for f in range(F)], [t.t().contiguous().t() for t in _as_list(x)]):
        assert _same(_run(lay, other, g), plain)


def _scores(case):
    X, (W, b, h, _) = case['X'].astype(np.float64), case['W']
    ii, jj = np.triu_indices(X.shape[1], 1)
    return np.maximum(X[:, ii] * X[:, jj] @ W.astype(np.float64) + b, 0.0) @ h.astype(np.float64).reshape(-1)


def _coarse_case(seed, B, F, D, A, proj, h_value):
    """Inputs whose scores are exactly representable: X in multiples of 1/4 up to 2, W and b in multiples of 1/8 up to 1/2, every h_a = h_value (an
    integer).  Every product and partial sum up to e is a multiple of 1/128 below 2^8, so an fp32 evaluation of e in any order is exact (a z of
    exactly 0 is shut in fp32 and fp64 alike)."""
    key = ('coarse', seed, B, F, D, A, proj, h_value)
    if key not in _CASES:
        rng = np.random.default_rng(seed)
        X = (rng.integers(-8, 9, (B, F, D)) / 4).astype(np.float32)
        W = (rng.integers(-4, 5, (D, A)) / 8).astype(np.float32)
        b = (rng.integers(-4, 5, A) / 8).astype(np.float32)
        h = np.full(A, h_value, np.float32)
        p = (rng.standard_normal(D) / np.sqrt(D)).astype(np.float32) if proj else None
        g = rng.standard_normal((B, 1 if proj else D)).astype(np.float32)
        _CASES[key] = _freeze(dict(X=X, W=(W, b, h, p), g=g, ref=O.run(X, W, b, h, p, g)))
    return _CASES[key]


@pytest.mark.parametrize('proj', [True, False], ids=['proj', 'pooled'])
def test_scores_of_magnitude_100(dev, proj):
    """projection_h = 11: the largest e is about 100 and most samples are near one-hot; nothing overflows and the 1e-5 bound holds.
    An fp32 e of magnitude L carries an absolute error of about L 2^-24 sqrt(D + A), which the exponential turns into the same RELATIVE error of
    the attention weights and of every dX row that is made of small weights only: at L = 60 .. 100 the plain fp32 composition is 0.9 to 1.9 times
    the bound on dX with draw's random inputs at (40, 8, 8, 4), (40, 8, 4, 2) and (40, 8, 4, 4) alike, so narrowing the shape does not help and
    the case uses inputs whose e is exactly representable instead (composition: 0.65 dX, 0.18 at most elsewhere)."""
    case = _coarse_case(7, 40, 8, 8, 4, proj, 11.0)
    e = _scores(case)
    assert 90 <= np.abs(e).max() <= 120
    a = case['ref']['a']
    assert np.median(a.max(1)) > 0.99
    best = min(max(a[s, k] for k, ij in enumerate(O.pairs(8)) if f in ij) for s in range(40) for f in range(8))
    assert best > 1e-33                                    # every dX row has a pair whose weight is a normal fp32 number
    got = _check(dev, case, 'scores of 100 %s' % ('proj' if proj else 'pooled'))
    assert all(bool(torch.isfinite(t).all()) for t in [got[0], got[1]] + got[2])


def test_the_maximum_at_every_pair_in_turn(dev):
    """F = 12, P = 66 (pairs 64 and 65 are a lane's SECOND pair), 66 samples: sample s has its maximum at pair s, at e >= 109, where exp overflows
    unless that pair takes part in the maximum.  An fp32 e of that size carries an absolute error of about 100 * 2^-24 * sqrt(terms) = 2e-5 and so
    cannot meet the 1e-5 bound on random inputs (the plain fp32 composition is 2 to 3.6 times over it on dX); this input is therefore exactly
    representable: X in {-1, 0, 1}, the two fields of pair s equal with entries +-2, W in {1/4, 1/2}, b = (28, 28, 28, -7/8), h = 1.  Every product
    and sum up to e is exact in fp32 in any order, and no z is 0.  The samples are near one-hot (second pair at e^-13 or less): dW, db and dh are
    sums of the small de, which the plain fp32 composition gets more than a thousand times the bound wrong (dW 1.7e3, dh 9e3 of it; v 0.009, dX 0.15)
    because its da_top - sum a da cancels; the kernel shifts da by da_top first."""
    B, F, D, A = 66, 12, 4, 4
    key = ('spike', B, F, D, A)
    if key not in _CASES:
        rng = np.random.default_rng(81)
        X = rng.integers(-1, 2, (B, F, D)).astype(np.float32)
        W = rng.choice([0.25, 0.5], (D, A)).astype(np.float32)
        b, h = np.array([28., 28., 28., -0.875], np.float32), np.ones(A, np.float32)
        for s, (i, j) in enumerate(O.pairs(F)):
            X[s, i] = 2.0 * rng.choice([-1.0, 1.0], D)
            X[s, j] = X[s, i]
        g = rng.standard_normal((B, D)).astype(np.float32)
        _CASES[key] = _freeze(dict(X=X, W=(W, b, h, None), g=g, ref=O.run(X, W, b, h, None, g)))
    case = _CASES[key]
    e = _scores(case)
    assert all(e[s].argmax() == s and e[s, s] > 89 and e[s, s] - np.delete(e[s], s).max() >= 13 for s in range(B))
    assert (e.max(1) - e.min(1)).max() < 60              # the smallest attention weight is far above the fp32 denormals
    assert O.gate_margin(case['X'], case['W'][0], case['W'][1]).min() >= 0.01
    got = _run(_layer(case, dev), torch.tensor(case['X']).to(dev), torch.tensor(case['g']).to(dev))
    assert all(bool(torch.isfinite(t).all()) for t in [got[0], got[1]] + got[2])
    _hold_all(got, case, 'maximum at every pair', db_cancels=True)      # units 0 .. 2 are open for every pair: their db cancels exactly


def _zero_edit(X, g):
    X[3] = 0.0
    X[7] = -0.0
    X[11, 2] = 0.0                                      # one field of a sample only
    g[5] = 0.0


def test_zero_rows_negative_zero_and_zeros_in_the_gradient(dev):
    for proj in (True, False):
        case = _case(31, 19, 5, 12, 4, proj, edit=_zero_edit)
        assert O.gate_margin(case['X'], case['W'][0], case['W'][1]).min() >= O.GATE
        out, dx, dws = _check(dev, case, 'zeros', three_d=True)
        assert float(out[3].abs().max()) == 0.0 and float(out[7].abs().max()) == 0.0
        assert float(dx[3].abs().max()) == 0.0 and float(dx[7].abs().max()) == 0.0 and float(dx[5].abs().max()) == 0.0
        assert float(dx[11, 2].abs().max()) > 0.0        # a zero field still receives a gradient
        assert all(bool(torch.isfinite(t).all()) for t in [out, dx] + dws)


@pytest.mark.parametrize('proj', [True, False], ids=['proj', 'pooled'])
def test_a_nan_stays_in_its_sample(dev, proj):
    case = _case(41, 70, 6, 16, 8, proj)
    lay = _layer(case, dev)
    x = torch.tensor(case['X']).to(dev)
    g = torch.tensor(case['g']).to(dev)
    clean = _run(lay, x, g)
    x = x.clone()
    x[33, 2, 5] = float('nan')
    dirty = _run(lay, x, g)
    keep = torch.ones(70, dtype=torch.bool, device=dev)
    keep[33] = False
    assert torch.equal(dirty[0][keep], clean[0][keep]) and bool(torch.isnan(dirty[0][33]).any())
    assert torch.equal(dirty[1][keep], clean[1][keep]) and bool(torch.isnan(dirty[1][33]).any())
    assert bool(torch.isnan(dirty[2][0]).any())


def test_frozen_weights_skip_dw_and_runs_repeat_bit_for_bit(dev):
    case = _case(51, 300, 9, 16, 8)
    x, g = torch.tensor(case['X']).to(dev), torch.tensor(case['g']).to(dev)
    lay = _layer(case, dev)
    first, second = _run(lay, x, g), _run(lay, x, g)
    assert _same(first, second)
    from rec_now_amd import _lib
    asked = []
    real = _lib.workspace
    _lib.workspace = lambda n, d: (asked.append(n), real(n, d))[1]
    try:
        again = _run(lay, x, g)
        assert len(asked) == 1 and asked[0] == _lib.load().recnow_afm_workspace_bytes(300, 9, 16, 8)
        frozen = _run(_layer(case, dev, trainable=False), x, g)
    finally:
        _lib.workspace = real
    assert frozen[2] is None and len(asked) == 1 and _same(again, first)
    assert torch.equal(frozen[0], first[0]) and torch.equal(frozen[1], first[1])


def test_graph_capture_replays_bit_for_bit(dev):
    case = _case(61, 129, 7, 16, 8)
    lay = _layer(case, dev)
    x = torch.tensor(case['X']).to(dev).requires_grad_(True)
    g = torch.tensor(case['g']).to(dev)

    def step():
        out = lay(x)
        return (out,) + torch.autograd.grad(out, [x] + _weights(lay), g)
    step()                                             # the pointer tables are uploaded (and cached) outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    rng = np.random.default_rng(62)
    for _ in range(2):
        with torch.no_grad():                          # new contents, same storage
            x.copy_(torch.from_numpy(rng.standard_normal(case['X'].shape).astype(np.float32)))
            g.copy_(torch.from_numpy(rng.standard_normal(case['g'].shape).astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        assert all(torch.equal(a, b) for a, b in zip(outs, eager))


@pytest.mark.parametrize('proj', [True, False], ids=['proj', 'pooled'])
def test_forward_allocates_only_its_output(dev, proj):
    from rec_now_amd.layers.afm_layer import AFMLayer
    B, F, D = 4096, 24, 16
    x = torch.randn(B, F, D, device=dev)
    lay = AFMLayer(16, projection=proj)
    with torch.no_grad():
        lay(x[:2].contiguous())
        lay(x)                                         # the pointer table of this call is uploaded once per content
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = lay(x)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    assert y.numel() == (B if proj else B * D)
    assert rise <= y.numel() * 4 + 4096, 'the forward allocated %d bytes above its output' % (rise - y.numel() * 4)


def test_pooled_vector_into_a_dense_head_matches_fp64_autograd(dev):
    """AFMLayer(projection=False) -> MultiDenseLayer: the output, dX and every parameter gradient against fp64 autograd of an einsum restatement."""
    import dense_ref as R
    from rec_now_amd.layers.afm_layer import AFMLayer
    from rec_now_amd.layers.multi_dense_layer import MultiDenseLayer
    torch.manual_seed(5)
    B, F, D = 48, 6, 8
    rng = np.random.default_rng(71)
    pool, head = AFMLayer(4, projection=False), MultiDenseLayer(4, 1)
    x = torch.from_numpy(rng.standard_normal((B, F, D)).astype(np.float32)).to(dev).requires_grad_(True)
    gy = torch.from_numpy(rng.standard_normal((B, 4)).astype(np.float32)).to(dev)
    y = head(pool(x)).reshape(B, 4)
    with torch.no_grad():
        pool.attention_b.copy_(torch.from_numpy((rng.standard_normal(4) * 0.1).astype(np.float32)))
    y = head(pool(x)).reshape(B, 4)
    params = {'afm/' + n: w for n, w in pool.named_weights().items()}
    params.update({'head/kernel': head.kernel, 'head/bias': head.bias})
    grads = torch.autograd.grad(y, [x] + list(params.values()), gy)
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in params.items()}
    x64 = x.detach().cpu().double().requires_grad_(True)
    assert O.gate_margin(x64.detach().numpy(), p64['afm/attention_W'].detach().numpy(), p64['afm/attention_b'].detach().numpy()).min() >= O.GATE
    ii, jj = np.triu_indices(F, 1)
    pk = x64[:, ii] * x64[:, jj]
    a = torch.softmax(torch.relu(pk @ p64['afm/attention_W'] + p64['afm/attention_b']) @ p64['afm/projection_h'][:, 0], -1)
    y64 = R.multi_dense_layer((a[..., None] * pk).sum(1), p64['head/kernel'], p64['head/bias']).reshape(B, 4)
    _hold('module out', y, y64.detach().numpy(), O.reltensor, 'module')
    g64 = torch.autograd.grad(y64, [x64] + list(p64.values()), gy.cpu().double())
    for name, got, want in zip(['x'] + list(params), grads, g64):
        _hold('module d ' + name, got, want.numpy(), O.reltensor, 'module')


def test_zz_report_the_worst_fractions():
    """Last in the file: the largest fraction of the 1e-5 bound seen per tensor by the tests above (printed; the bound itself is asserted there)."""
    for what in sorted(WORST):
        print('worst %-24s %.3f of the bound' % (what, WORST[what]))
    assert all(v <= 1.0 for v in WORST.values())
