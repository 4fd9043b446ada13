"""The CINLayer census (tests/_cin_census.py) has teeth, without a GPU: every row of the route table (tests/_cin_routes.py) gets census data whose
every sum stays inside the 2^24 window, so fp32 restatements of the stack in three summation orders -- in the kernels' factorisation, fused form
and two products -- equal the exact result bit for bit in every mode the row runs in; every listed kernel mistake that applies to the row moves at
least one checked output; the exact result equals the fp64 autograd of oracle/dense_ref.cin_layer; the restated route predicate gives the route
the row names."""
import numpy as np
import pytest
import torch

import _cin_census as C
import _cin_routes as T
import dense_ref as R
from _cin_routes import ROUTES, MISALIGNED, spec

_CACHE = {}
ALL = ROUTES + [MISALIGNED]


def _census(r):
    key = (tuple(sorted(spec(r).items())), r['modes'])
    if key not in _CACHE:
        _CACHE[key] = C.make(modes=r['modes'], **spec(r))
    c = _CACHE[key]
    assert c.params == r['census'], '%s: the table says census parameters %r, the ladder picks %r' % (r['name'], r['census'], c.params)
    return c


def _same(what, got, want):
    got = np.asarray(got, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1).view(np.int32) != want.astype(np.float32).reshape(-1).view(np.int32))
    assert bad.size == 0, '%s: %d of %d differ, first flat %d: %r vs %r' % (what, bad.size, want.size, bad[0], got.reshape(-1)[bad[0]],
                                                                          want.reshape(-1)[bad[0]])


@pytest.mark.parametrize('r', ALL, ids=[r['name'] for r in ALL])
def test_row_census_is_exact(r):
    c = _census(r)          # C.make has checked the window and the fp32 intermediates in every mode of the row
    fused = r['fused'] if r is MISALIGNED else None
    for oi, sc in r['modes']:
        want = C.expected(c, oi, sc)
        assert set(C.checked(c)) <= set(want)
        for name, order in C.ORDERS.items():
            got = C.restate(c, oi, sc, order=order, fused=fused)
            for k in want:
                _same('%s %s mode %d%d %s' % (r['name'], name, oi, sc, k), got[k], want[k])
        # not degenerate: most outputs carry nonzero values (demb: on the rows with a gradient), every dW_k has nonzeros
        on = np.repeat(c.on.reshape(r['B'], 1, r['D']), r['F'], 1).reshape(r['B'], -1)
        assert np.count_nonzero(want['out']) > 0.5 * want['out'].size
        assert np.count_nonzero(want['demb'][on]) > 0.5 * on.sum() and not want['demb'][~on].any()
        for l in range(len(r['Hs'])):
            assert np.count_nonzero(want['dW%d' % l]) > 0, 'dW%d is all zero' % l


@pytest.mark.parametrize('r', ALL, ids=[r['name'] for r in ALL])
def test_row_catches_every_mutation(r):
    c = _census(r)
    fused = r['fused'] if r is MISALIGNED else None
    for oi, sc in r['modes']:
        clean = C.restate(c, oi, sc, fused=fused)
        for mut, (what, applies) in C.MUTATIONS.items():
            if r is MISALIGNED and mut in ('parity_lost', 'drop_last_column_tile', 'drop_last_ktile', 'ri_permuted'):
                continue                                   # nothing of this row runs on the fused kernel
            if not applies(spec(r), oi, sc):
                continue
            bad = C.restate(c, oi, sc, mut=mut, fused=fused)
            moved = [k for k in C.checked(c) if not np.array_equal(clean[k], bad[k])]
            assert moved, '%s mode %d%d: mutation %r (%s) changes no checked output' % (r['name'], oi, sc, mut, what)


def test_every_mutation_applies_somewhere():
    for mut, (what, applies) in C.MUTATIONS.items():
        assert any(applies(spec(r), oi, sc) for r in ROUTES for oi, sc in r['modes']), mut


@pytest.mark.parametrize('r', ALL, ids=[r['name'] for r in ALL])
def test_row_route_predicate(r):
    """the restated rn_cin_bwd_fused_supported and pick_cfg give the route the row names"""
    assert T.fused_layers(r['B'], r['D'], r['F'], r['Hs'], aligned=r is not MISALIGNED) == r['fused'], r['name']
    assert T.fwd_tags(r['Hs']) == r['tags'], r['name']


def test_route_predicate_corners():
    assert T.cb_lds_bytes(92) <= 160 * 1024 < T.cb_lds_bytes(96) and T.cb_lds_bytes(92) == 160000
    assert T.fused_supported(128, 32, 64, 92) and not T.fused_supported(128, 32, 64, 96)
    assert not T.fused_supported(128, 32, 64, 6) and not T.fused_supported(128, 32, 64, 2)
    assert [T.pick_cfg(n) for n in (16, 32, 33, 64, 65, 128, 129, 160, 161)] == [
        (256, 32), (256, 32), (256, 64), (256, 64), (128, 128), (128, 128), (128, 160), (128, 160), (128, 128)]
    assert T.bwd_launches((False, True, True)) == 5
    names = {r['name'] for r in ROUTES}
    fused_hp = {([r['F']] + list(r['Hs']))[k] for r in ROUTES for k, f in enumerate(r['fused']) if f}
    assert fused_hp == {64, 128} and len(names) == len(ROUTES)


@pytest.mark.parametrize('r', [r for r in ALL if r['B'] * r['D'] <= 256 and r['F'] <= 64], ids=lambda r: r['name'])
def test_expected_is_the_reference_layer(r):
    """at the small shapes `expected` equals oracle/dense_ref.cin_layer with fp64 autograd, on the same data"""
    c = _census(r)
    for oi, sc in r['modes']:
        want = C.expected(c, oi, sc)
        x = torch.from_numpy(c.emb).double().requires_grad_(True)
        ws = [torch.from_numpy(w).double().reshape(1, 1, *w.shape).requires_grad_(True) for w in c.W]
        y = R.cin_layer(x, ws, r['F'], r['D'], bool(oi), bool(sc))
        y.backward(torch.from_numpy(c.dout(oi, sc)).double())
        assert np.array_equal(y.detach().numpy(), want['out'])
        assert np.array_equal(x.grad.numpy(), want['demb'])
        for l, w in enumerate(ws):
            assert np.array_equal(w.grad.numpy().reshape(c.W[l].shape), want['dW%d' % l]), 'dW%d' % l


def test_gradient_rows():
    on = C.grad_rows(32896, 64)
    assert on[0] and on[-1] and on.reshape(257, 128).any(1).all() and 0.01 < on.mean() < 0.04
    assert C.grad_rows(2048, 64).all()


def test_weights_are_not_symmetric():
    c = _census(ROUTES[1])                                   # H_0 = F = 64: a swapped (f, h) is a transpose of the 64 x 64 column grid
    W = c.W[0].reshape(32, 64, 64)
    assert not np.array_equal(W, W.transpose(0, 2, 1)) and set(np.unique(np.abs(W))) == {0.0, 1.0}
    assert (np.count_nonzero(c.W[0], axis=1) == c.params[0]).all()


def test_fused_constant():
    """the per-product constant of the fused kernel on random data (tests/_cin_census.py C_FUSED) covers a host fp32 emulation of its
    summation orders at the shapes of the rows, with the margin the GEMM constant has"""
    worst = 0.0
    for r in ROUTES:
        ext = [r['F']] + list(r['Hs'])
        for k, f in enumerate(r['fused']):
            if f:
                worst = max(worst, C.fused_constant(ext[k + 1], ext[k], r['F'], rows=128))
    print('fused kernel: max |emulation - fp64| / sum |terms| = %.3g' % worst)
    assert worst <= C.C_FUSED_MEASURED and C.C_FUSED == 2.4 * C.C_FUSED_MEASURED


def test_window_shrinks_the_data_where_needed():
    """six layers grow the activations by (k xmax)^6: the first parameters do not fit, the ladder shrinks them and the result holds the invariant"""
    c = C.make(B=2, D=4, F=4, Hs=(32,) * 6)
    assert c.params != C.LADDER[0]
    for oi, sc in T.ALL4:
        C.check_invariant(c, oi, sc)
    with pytest.raises(AssertionError):
        C.make(B=2, D=4, F=4, Hs=(32,) * 6, params=C.LADDER[0])


def test_invariant_is_enforced():
    c = C.make(B=8, D=16, F=4, Hs=(64, 32))
    c.emb = c.emb * np.float32(4096.0)
    c.__dict__.pop('_fw', None)
    with pytest.raises(AssertionError):
        C.check_invariant(c, 1, 1)
