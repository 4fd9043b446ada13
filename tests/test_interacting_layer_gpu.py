"""GPU: InteractingLayer (csrc/autoint.hip) against the fp64 oracle of tests/_autoint_oracle.py, on every route and access width.

Bound: the project's 1e-5.  `out` and every field's dX are held per row (error <= 1e-5 of that row's largest fp64 magnitude; a row of `out` is
a sample's F*E values, a row of dX one field of one sample), each dW against its tensor's largest magnitude.  Inputs: unit-variance X, weights of
std 1/sqrt(D), a unit-variance upstream gradient; samples within 2e-5 of the ReLU kink are redrawn (_autoint_oracle.draw), so no entry is left
out of any comparison.  On the shapes below the plain fp32 torch composition on the CPU stays within 7.1e-7 (out), 2.8e-6 (dX) and 8.5e-7 (dW)
of the oracle on these measures, so the bound leaves about 3.5x headroom over plain fp32.  The large-logit case is the exception: with X scaled
by 3 (largest |logit| about 100) the fp32 composition sits at 0.11 (out), 0.56 (dX) and 0.14 (dW) of the bound at (40, 8, 8, 2, 4), and at 0.98
(dX) at D 16, d 8 -- an fp32 logit of magnitude L carries an absolute error of about L * 2^-24 * sqrt(D + d), which the exponential turns into
the same RELATIVE error of the attention weights; the case therefore uses the narrower shape.
Every comparison prints its fraction of the bound; the largest per tensor are printed once more by the last test of the file."""
import os
import re

import numpy as np
import pytest
import torch

import _autoint_oracle as O

pytestmark = pytest.mark.gpu
RTOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (B, F, D, H, d): a single field; nothing divisible by 4; ..; more fields than a 16-lane group, d = 2; the benchmark shape; the F limit; the D, E
# and H limits (the backward's weights and accumulators do not fit LDS); odd everything, weights read through L2 with 4-byte accesses; B = 1 and
# d = 1; one wide head; and weights read through L2 with 16-byte accesses in both directions
SHAPES = [(3, 1, 4, 1, 4), (5, 2, 5, 1, 3), (37, 8, 16, 2, 8), (130, 17, 8, 4, 2), (67, 24, 16, 2, 8), (9, 64, 4, 1, 4), (33, 6, 64, 8, 8),
          (2, 40, 63, 7, 9), (1, 7, 16, 2, 1), (70, 3, 20, 1, 64), (3, 40, 64, 8, 8)]
WORST = {}
NAMES = ('W_query', 'W_key', 'W_value', 'W_res')
_CASES = {}


def _consts():
    src = open(os.path.join(ROOT, 'rec_now_amd', 'csrc', 'autoint.hip')).read()
    return {k: int(v) for k, v in re.findall(r'#define (AI_[A-Z_]+) \(?(\d+)\)?\s', src)}


def _case(seed, B, F, D, H, d, use_res=True, scaling=False, relu=True, x_scale=1.0, edit=None):
    """Inputs and their fp64 results, computed once per distinct case and shared by the tests."""
    key = (seed, B, F, D, H, d, use_res, scaling, relu, x_scale, edit)
    if key not in _CASES:
        X, Wq, Wk, Wv, Wr, g = O.draw(np.random.default_rng(seed), B, F, D, H, d, use_res, scaling, x_scale)
        if edit is not None:
            edit(X, g)
        ref = O.run(X, Wq, Wk, Wv, Wr, H, d, scaling, relu, g)
        for a in (X, Wq, Wk, Wv, g) + ((Wr,) if use_res else ()):
            a.setflags(write=False)
        _CASES[key] = dict(X=X, W=(Wq, Wk, Wv, Wr), g=g, ref=ref, cfg=(H, d, use_res, scaling, relu))
    return _CASES[key]


def _layer(case, dev, trainable=True):
    from rec_now_amd.layers.interacting_layer import InteractingLayer
    H, d, use_res, scaling, relu = case['cfg']
    lay = InteractingLayer(d, H, use_res=use_res, scaling=scaling, activation='relu' if relu else None, trainable=trainable)
    lay._build_device = dev
    lay.build(case['X'].shape)
    lay.set_weights_by_name({n: w.copy() for n, w in zip(NAMES, case['W']) if w is not None})
    return lay


def _weights(lay):
    return [w for w in (lay.W_query, lay.W_key, lay.W_value, lay.W_res) if w is not None]


def _as_list(x):
    return [x[:, f].contiguous() for f in range(x.shape[1])]


def _run(lay, inputs, g):
    """One forward + backward.  inputs: a (B, F, D) tensor or a list of (B, D).  Returns (out, dX stacked (B, F, D), [dW] or None)."""
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


def _check(dev, case, key, three_d=False):
    """Runs the layer on the case and holds out, every field's dX and every dW to the fp64 oracle."""
    lay = _layer(case, dev)
    x = torch.tensor(case['X']).to(dev)
    got = _run(lay, x if three_d else _as_list(x), torch.tensor(case['g']).to(dev))
    ref = case['ref']
    B, F, D = case['X'].shape
    assert got[0].dtype == torch.float32 and tuple(got[0].shape) == ((B, F, ref['out'].shape[2]) if three_d else (B, F * ref['out'].shape[2]))
    _hold('out', got[0], ref['out'], O.relrow, key)
    _hold('dX', got[1].reshape(B * F, D), ref['dX'].reshape(B * F, D), O.relrow, key)
    for name, dw in zip([n for n, w in zip(NAMES, case['W']) if w is not None], got[2]):
        _hold('d' + name, dw, ref['d' + name.replace('_query', 'q').replace('_key', 'k').replace('_value', 'v').replace('_res', 'r')], O.reltensor, key)
    return got


def _same(a, b):
    return torch.equal(a[0].reshape(-1), b[0].reshape(-1)) and torch.equal(a[1], b[1]) and (
        (a[2] is None and b[2] is None) or all(torch.equal(p, q) for p, q in zip(a[2], b[2])))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'B%d-F%d-D%d-H%d-d%d' % s)
def test_matches_the_oracle(dev, shape):
    B, F, D, H, d = shape
    _check(dev, _case(B * 1000 + F * 10 + D, *shape), str(shape))


@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'linear'])
@pytest.mark.parametrize('scaling', [False, True], ids=['raw', 'scaled'])
@pytest.mark.parametrize('use_res', [True, False], ids=['res', 'nores'])
def test_every_setting(dev, use_res, scaling, relu):
    _check(dev, _case(5, 21, 7, 12, 3, 4, use_res, scaling, relu), 'res %d scaling %d relu %d' % (use_res, scaling, relu), three_d=True)


def test_more_samples_than_workgroup_slots_and_a_ragged_last_batch(dev):
    """More samples than AI_MAXG workgroups of AI_DW_ROWS take in one batch of waves: every workgroup walks several batches, and the last
    workgroup ends on a batch with fewer samples than waves."""
    c = _consts()
    B = c['AI_MAXG'] * c['AI_DW_ROWS'] + 4 * c['AI_MAXG'] + 37
    rows = -(-(-(-B // c['AI_MAXG'])) // 4) * 4                  # samples per workgroup: ceil(B / G) rounded up to the 4 waves
    assert rows >= 8 and B % rows != 0 and (B % rows) % 4 != 0
    _check(dev, _case(11, B, 3, 4, 1, 4), '(%d, 3, 4, 1, 4)' % B)


def test_every_route_is_reached(dev):
    """Every (route, access width, direction) the dispatcher and the kernels can pick is reached by a case of test_matches_the_oracle: weights
    (and weight-gradient accumulators) resident in LDS or behind L2; 16-byte accesses (D % 4 == 0 and E % 4 == 0) and guarded 4-byte ones."""
    from rec_now_amd import _lib
    lib = _lib.load()
    seen = set()
    for (B, F, D, H, d) in SHAPES:
        for bwd in (0, 1):
            seen.add((lib.recnow_autoint_route(F, D, H, d, 1, bwd), D % 4 == 0 and (H * d) % 4 == 0, bwd))
    assert seen == {(r, v, b) for r in (0, 1) for v in (False, True) for b in (0, 1)}
    assert any(D % 4 == 0 and (H * d) % 4 != 0 for _, _, D, H, d in SHAPES)                 # mixed widths: X by 16 bytes, out by 4
    assert any(B > _consts()['AI_DW_ROWS'] * 4 for B, _, _, _, _ in SHAPES) and any(B == 1 for B, _, _, _, _ in SHAPES)


def test_empty_batch(dev):
    from rec_now_amd.layers.interacting_layer import InteractingLayer
    lay = InteractingLayer(4, 2)
    xs = [torch.zeros(0, 8, device=dev, requires_grad=True) for _ in range(3)]
    out = lay(xs)
    assert tuple(out.shape) == (0, 3 * 8)
    grads = torch.autograd.grad(out, xs + _weights(lay), torch.zeros_like(out))
    assert all(tuple(a.shape) == (0, 8) for a in grads[:3]) and all(float(a.abs().max()) == 0.0 and tuple(a.shape) == (8, 8) for a in grads[3:])
    x3 = torch.zeros(0, 3, 8, device=dev, requires_grad=True)
    out3 = lay(x3)
    assert tuple(out3.shape) == (0, 3, 8) and tuple(torch.autograd.grad(out3, [x3], torch.zeros_like(out3))[0].shape) == (0, 3, 8)


def test_single_field_is_a_dense_layer(dev):
    case = _case(3003, 3, 1, 4, 1, 4)
    lay = _layer(case, dev)
    x = torch.tensor(case['X']).to(dev)
    want = torch.relu(x[:, 0].double() @ (lay.W_value.double() + lay.W_res.double()))
    assert O.relrow(lay([x[:, 0]]).detach().cpu().numpy(), want.detach().cpu().numpy()) <= RTOL


def test_layouts_agree_bit_for_bit(dev):
    """A list of contiguous fields, a (B, F, D) tensor, column views of a (B, F*D) tensor and storage that starts one float into an allocation
    (4-byte accesses) give the same bits."""
    case = _case(21, 41, 6, 8, 2, 4)
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


def test_logits_of_magnitude_100(dev):
    """X scaled by 3: the largest |logit| is about 100 and most attention rows are near one-hot; nothing overflows and the 1e-5 bound holds."""
    case = _case(7, 40, 8, 8, 2, 4, x_scale=3.0)
    X, (Wq, Wk, _, _) = case['X'].astype(np.float64), case['W']
    S = np.einsum('bihc,bjhc->bhij', (X @ Wq).reshape(40, 8, 2, 4), (X @ Wk).reshape(40, 8, 2, 4))
    assert 80 <= np.abs(S).max() <= 150
    P = np.exp(S - S.max(-1, keepdims=True))
    assert np.median((P / P.sum(-1, keepdims=True)).max(-1)) > 0.99
    got = _check(dev, case, 'logits of 100')
    assert all(bool(torch.isfinite(t).all()) for t in [got[0], got[1]] + got[2])


def test_the_row_maximum_on_every_lane_in_turn(dev):
    """W_query = W_key = I and field b % F of sample b scaled by 6: query b % F has a logit of about 36 |x|^2 = 290 at its own key and about +-17
    elsewhere, so exp overflows unless that key's lane takes part in the row maximum -- for every lane 0 .. F-1 in turn."""
    B, F, D, H, d = 24, 8, 8, 1, 8
    key = ('spike', B, F, D, H, d)
    if key not in _CASES:
        rng = np.random.default_rng(81)
        X, _, _, Wv, Wr, g = O.draw(rng, B, F, D, H, d)
        for b in range(B):
            X[b, b % F] *= 6.0
        eye = np.eye(D, dtype=np.float32)
        ref = O.run(X, eye, eye, Wv, Wr, H, d, False, True, g)
        _CASES[key] = dict(X=X, W=(eye, eye.copy(), Wv, Wr), g=g, ref=ref, cfg=(H, d, True, False, True))
    case = _CASES[key]
    X64 = case['X'].astype(np.float64)
    S = np.einsum('bic,bjc->bij', X64, X64)
    assert all(S[b, b % F, b % F] - np.delete(S[b, b % F], b % F).max() > 89 for b in range(B))       # exp(89) is past the fp32 range
    assert case['ref']['ratio'].min() >= O.KINK
    got = _run(_layer(case, dev), torch.tensor(case['X']).to(dev), torch.tensor(case['g']).to(dev))
    assert all(bool(torch.isfinite(t).all()) for t in [got[0], got[1]] + got[2])
    ref = case['ref']
    _hold('out', got[0], ref['out'], O.relrow, 'maximum on every lane')
    for name, dw in zip(('dWq', 'dWk', 'dWv', 'dWr'), got[2]):
        _hold('dW_spike', dw, ref[name], O.reltensor, 'maximum on every lane')
    # dX is held to 1e-4 here: X carries a factor 6 and logits of 290, whose fp32 rounding (290 * 2^-24 * sqrt(D) = 5e-5) reaches the weights of
    # competing keys; the plain fp32 torch composition is 1.6e-5 off on this input
    frac = O.relrow(got[1].reshape(B * F, D).cpu().numpy(), ref['dX'].reshape(B * F, D)) / 1e-4
    print('maximum on every lane dX: %.3f of 1e-4' % frac)
    assert frac <= 1.0


def _zero_edit(X, g):
    X[3] = 0.0
    X[7] = -0.0
    X[11, 2] = 0.0                                      # one field of a sample only
    g[5] = 0.0
    g[:, :, ::3] = 0.0


def test_zero_rows_negative_zero_and_zeros_in_the_gradient(dev):
    case = _case(31, 19, 5, 12, 2, 4, edit=_zero_edit)
    ratio = case['ref']['ratio']
    assert ratio[11] >= O.KINK and ratio[3] == 1.0       # the edited sample is still off the kink; all-zero samples sit ON it: subgradient 0
    out, dx, dws = _check(dev, case, 'zeros')
    assert float(out[3].abs().max()) == 0.0 and float(out[7].abs().max()) == 0.0
    assert float(dx[3].abs().max()) == 0.0 and float(dx[7].abs().max()) == 0.0 and float(dx[5].abs().max()) == 0.0
    assert all(bool(torch.isfinite(t).all()) for t in [out, dx] + dws)


@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'linear'])
def test_a_nan_stays_in_its_sample(dev, relu):
    case = _case(41, 70, 6, 16, 2, 8, relu=relu)
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
    assert all(bool(torch.isnan(w).any()) for w in dirty[2])


def test_frozen_weights_skip_dw_and_runs_repeat_bit_for_bit(dev):
    case = _case(51, 300, 9, 16, 2, 8)
    x, g = torch.tensor(case['X']).to(dev), torch.tensor(case['g']).to(dev)
    lay = _layer(case, dev)
    first, second = _run(lay, x, g), _run(lay, x, g)
    assert _same(first, second)
    from rec_now_amd import _lib
    asked = []
    real = _lib.workspace
    _lib.workspace = lambda n, d: (asked.append(n), real(n, d))[1]
    try:
        frozen = _run(_layer(case, dev, trainable=False), x, g)
    finally:
        _lib.workspace = real
    assert frozen[2] is None and asked == []
    assert torch.equal(frozen[0], first[0]) and torch.equal(frozen[1], first[1])


def test_graph_capture_replays_bit_for_bit(dev):
    case = _case(61, 129, 7, 16, 2, 8)
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


def test_forward_allocates_only_its_output(dev):
    from rec_now_amd.layers.interacting_layer import InteractingLayer
    B, F, D = 4096, 24, 16
    x = torch.randn(B, F, D, device=dev)
    lay = InteractingLayer(8, 2)
    with torch.no_grad():
        lay(x[:2].contiguous())
        lay(x)                                         # the pointer table of this call is uploaded once per content
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = lay(x)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    assert y.numel() * 4 == B * F * 16 * 4
    assert rise <= y.numel() * 4 + 4096, 'the forward allocated %d bytes above its output' % (rise - y.numel() * 4)


def test_two_stacked_layers_and_a_dense_head_match_fp64_autograd(dev):
    """InteractingLayer -> InteractingLayer on the 3-D path (no copy between them) -> MultiDenseLayer: the output, dX and every parameter
    gradient against fp64 autograd of an einsum restatement."""
    import dense_ref as R
    from rec_now_amd.layers.interacting_layer import InteractingLayer
    from rec_now_amd.layers.multi_dense_layer import MultiDenseLayer
    torch.manual_seed(5)
    B, F, D = 48, 6, 8
    rng = np.random.default_rng(71)
    X = rng.standard_normal((B, F, D)).astype(np.float32)
    first, second, head = InteractingLayer(4, 2), InteractingLayer(3, 2, scaling=True), MultiDenseLayer(4, 1)
    x = torch.from_numpy(X).to(dev).requires_grad_(True)
    gy = torch.from_numpy(rng.standard_normal((B, 4)).astype(np.float32)).to(dev)
    y = head(second(first(x)).reshape(B, -1)).reshape(B, 4)
    params = {'l0/' + n: w for n, w in first.named_weights().items()}
    params.update({'l1/' + n: w for n, w in second.named_weights().items()})
    params.update({'head/kernel': head.kernel, 'head/bias': head.bias})
    grads = torch.autograd.grad(y, [x] + list(params.values()), gy)
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in params.items()}
    x64 = torch.from_numpy(X).double().requires_grad_(True)

    def attend(z, pre, H, d, scale):
        Q, K, V = ((z @ p64[pre + n]).reshape(B, F, H, d) for n in ('W_query', 'W_key', 'W_value'))
        A = torch.softmax(torch.einsum('bihc,bjhc->bhij', Q, K) * scale, -1)
        p = torch.einsum('bhij,bjhc->bihc', A, V).reshape(B, F, H * d) + z @ p64[pre + 'W_res']
        assert float(O.kink_ratio(p.detach().numpy()).min()) >= O.KINK          # off the ReLU kink in both layers
        return torch.relu(p)
    z = attend(attend(x64, 'l0/', 2, 4, 1.0), 'l1/', 2, 3, 3 ** -0.5)
    y64 = R.multi_dense_layer(z.reshape(B, -1), p64['head/kernel'], p64['head/bias']).reshape(B, 4)
    _hold('module out', y, y64.detach().numpy(), O.reltensor, 'module')
    g64 = torch.autograd.grad(y64, [x64] + list(p64.values()), gy.cpu().double())
    for name, got, want in zip(['x'] + list(params), grads, g64):
        _hold('module d ' + name, got, want.numpy(), O.reltensor, 'module')


def test_zz_report_the_worst_fractions():
    """Last in the file: the largest fraction of the 1e-5 bound seen per tensor by the tests above (printed; the bound itself is asserted there)."""
    for what in sorted(WORST):
        print('worst %-24s %.3f of the bound' % (what, WORST[what]))
    assert all(v <= 1.0 for v in WORST.values())
