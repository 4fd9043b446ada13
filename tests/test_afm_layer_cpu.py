"""CPU: the fp64 oracle of AFMLayer is pinned (a hand-worked example, an independent einsum restatement under fp64 autograd, and the identities
of the definition), the input generator's redraw rate is held to its estimate, and the host side of the layer is covered: constructor and shape
errors, weight names and shapes, the library's `supported`, `route` and `workspace_bytes` queries, the ABI version, and the refusal of CPU
tensors.

Redraw rate: a sample is redrawn when one of its P A hidden values has |z| < 1e-5 (sum_c |W_ca p_c| + |b_a|).  z is roughly normal with a
standard deviation of 0.3 to 1 of that sum / sqrt(D) .. that sum, so one value lands there with probability 1e-5 to 3e-5 and a sample with about
1 - exp(-(1 .. 3)e-5 P A); the test holds the rate to the upper end, 3e-5 P A, at the shapes the GPU tests draw."""
import os
import re

import numpy as np
import pytest
import torch

import _afm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = np.log(2.0)


def _layer(*a, **k):
    from rec_now_amd.layers.afm_layer import AFMLayer
    return AFMLayer(*a, **k)


def _consts():
    src = open(os.path.join(ROOT, 'rec_now_amd', 'csrc', 'afm.hip')).read()
    return {k: int(v) for k, v in re.findall(r'#define (AFM_[A-Z_]+) \(?(\d+)\)?\s', src)}


# ---- the oracle ------------------------------------------------------------------------------------------------------------------

def test_oracle_matches_a_hand_worked_example():
    """F = 3, D = 2, A = 1: x0 = (1, 2), x1 = (1, 0), x2 = (0, 1); W = (ln 2, -1)^T, b = ln 2, h = 1, p = (7, 7).
    p_01 = (1, 0), p_02 = (0, 2), p_12 = (0, 0);  z = (2 ln 2, ln 2 - 2, ln 2);  e = (2 ln 2, 0, ln 2);  a = (4, 1, 2) / 7;
    v = (4/7, 2/7);  out = 6."""
    X = np.array([[[1., 2.], [1., 0.], [0., 1.]]])
    W, b, h, p = np.array([[LN2], [-1.]]), np.array([LN2]), np.array([1.]), np.array([7., 7.])
    r = O.run(X, W, b, h, p, g=np.array([[1.]]))
    assert np.allclose(r['a'][0], [4. / 7, 1. / 7, 2. / 7], rtol=0, atol=1e-15)
    assert np.allclose(r['v'][0], [4. / 7, 2. / 7], rtol=0, atol=1e-15) and r['out'][0, 0] == pytest.approx(6.0, abs=1e-14)
    assert r['scale'][0] == pytest.approx(6.0, abs=1e-14)
    # backward with g = 1: dv = (7, 7); da = (7, 14, 0); sum a da = 6; de = (4, 8, -12) / 7; the middle pair is cut by the ReLU.
    # dh = de_0 2 ln 2 + de_2 ln 2 = -4/7 ln 2;  dz = (4/7, 0, -12/7);  db = -8/7;  dW = p_01 4/7 + p_12 (-12/7) = (4/7, 0);  dp = v
    assert np.allclose(r['dh'], [-4. / 7 * LN2], atol=1e-15) and np.allclose(r['db'], [-8. / 7], atol=1e-15)
    assert np.allclose(r['dW'][:, 0], [4. / 7, 0.], atol=1e-15) and np.allclose(r['dp'], [4. / 7, 2. / 7], atol=1e-15)
    # dp_01 = (4, 4) + (ln 2, -1) 4/7;  dp_02 = (1, 1);  dp_12 = (2, 2) - (ln 2, -1) 12/7
    assert np.allclose(r['dX'][0, 0], [4. + 4. / 7 * LN2, 1.], atol=1e-14)                  # dp_01 * x1 + dp_02 * x2
    assert np.allclose(r['dX'][0, 1], [4. + 4. / 7 * LN2, 74. / 7], atol=1e-14)             # dp_01 * x0 + dp_12 * x2
    assert np.allclose(r['dX'][0, 2], [3. - 12. / 7 * LN2, 2.], atol=1e-14)                 # dp_02 * x0 + dp_12 * x1


def _compose(X, W, b, h, p):
    F = X.shape[1]
    ii, jj = np.triu_indices(F, 1)
    pk = X[:, ii] * X[:, jj]
    a = torch.softmax(torch.relu(pk @ W + b) @ h, -1)
    v = (a[..., None] * pk).sum(1)
    return v if p is None else (v @ p)[:, None]


@pytest.mark.parametrize('projection', [True, False])
def test_oracle_matches_fp64_autograd_of_an_einsum_restatement(projection):
    B, F, D, A = 6, 5, 7, 3
    X, W, b, h, p, g = O.draw(np.random.default_rng(3), B, F, D, A, projection)
    r = O.run(X, W, b, h, p, g)
    t = [torch.tensor(a, dtype=torch.float64, requires_grad=True) if a is not None else None for a in (X, W, b, h, p)]
    out = _compose(*t)
    leaves = [a for a in t if a is not None]
    grads = torch.autograd.grad(out, leaves, torch.tensor(g, dtype=torch.float64))
    assert O.reltensor(r['out'], out.detach().numpy()) <= 1e-12
    for name, got in zip(['dX', 'dW', 'db', 'dh'] + (['dp'] if projection else []), grads):
        assert O.reltensor(r[name], got.numpy()) <= 1e-12, name
    assert projection or r['dp'] is None


def test_zero_projection_h_gives_uniform_attention_and_fm():
    """h = 0: e = 0, a = 1 / P, and P v is FM's second-order vector 1/2 ((sum x)^2 - sum x^2)."""
    X, W, b, h, _, _ = O.draw(np.random.default_rng(4), 5, 6, 4, 3, False)
    r = O.run(X, W, b, np.zeros_like(h))
    X64 = X.astype(np.float64)
    fm = 0.5 * (X64.sum(1) ** 2 - (X64 ** 2).sum(1))
    assert np.abs(r['a'] - 1.0 / 15).max() <= 1e-15 and np.abs(15 * r['v'] - fm).max() <= 1e-13


def test_two_fields_and_a_single_field():
    X, W, b, h, p, g = O.draw(np.random.default_rng(5), 7, 2, 5, 4, False)
    r = O.run(X, W, b, h, None, g)
    X64 = X.astype(np.float64)
    assert np.array_equal(r['a'], np.ones((7, 1))) and np.array_equal(r['v'], X64[:, 0] * X64[:, 1])
    assert not r['dW'].any() and not r['db'].any() and not r['dh'].any()
    assert np.abs(r['dX'][:, 0] - g * X64[:, 1]).max() <= 1e-15 and np.abs(r['dX'][:, 1] - g * X64[:, 0]).max() <= 1e-15
    one = O.run(X[:, :1], W, b, h, None, g)
    assert not one['out'].any() and not one['dX'].any() and not one['dW'].any()


def test_permuting_the_fields_changes_nothing_but_the_order_of_dx():
    X, W, b, h, p, g = O.draw(np.random.default_rng(6), 4, 6, 5, 3)
    perm = np.array([3, 0, 5, 1, 4, 2])
    a, c = O.run(X, W, b, h, p, g), O.run(X[:, perm], W, b, h, p, g)
    assert np.abs(a['out'] - c['out']).max() <= 1e-13 and np.abs(a['dX'][:, perm] - c['dX']).max() <= 1e-12
    assert np.abs(a['dW'] - c['dW']).max() <= 1e-12 and np.abs(a['dh'] - c['dh']).max() <= 1e-12


def test_projection_is_a_dot_product_after_the_pooling():
    X, W, b, h, p, g = O.draw(np.random.default_rng(7), 4, 5, 6, 3)
    proj = O.run(X, W, b, h, p, g)
    plain = O.run(X, W, b, h, None, g * p.astype(np.float64))           # dv = g p
    assert np.abs(proj['out'][:, 0] - plain['out'] @ p.astype(np.float64)).max() <= 1e-14
    assert np.abs(proj['dX'] - plain['dX']).max() <= 1e-13 and np.abs(proj['dW'] - plain['dW']).max() <= 1e-13
    assert np.abs(proj['dp'] - (g.astype(np.float64) * plain['out']).sum(0)).max() <= 1e-13


def test_measures():
    ref = np.array([[1., 0.], [1000., 0.]])
    assert O.relrow(ref + np.array([[0., 0.], [0., 1.]]), ref) == pytest.approx(1e-3)
    assert O.relrow(np.full((2, 2), np.nan), ref) == float('inf')
    assert O.relscale(np.array([[1.5]]), np.array([[1.0]]), np.array([5.0])) == pytest.approx(0.1)
    assert O.gate_margin(np.array([[[1., 1.], [1., 2.]]]), np.array([[1.], [-1.]]), np.array([1.]))[0] == pytest.approx(0.0)      # z = 1 - 2 + 1


@pytest.mark.parametrize('B,F,D,A', [(2000, 24, 16, 16), (1000, 64, 4, 4), (2000, 12, 64, 64), (1000, 17, 8, 5)])
def test_redraw_rate(B, F, D, A):
    """The rate at the shapes of the GPU tests, held to the upper estimate 3e-5 P A (see the docstring of the file)."""
    count = []
    X, W, b, _, _, _ = O.draw(np.random.default_rng(1), B, F, D, A, count=count)
    redrawn, drawn = count[0]
    P = F * (F - 1) // 2
    print('P*A %d: %d of %d samples redrawn (%.1f %%), estimate at most %.1f %%' % (P * A, redrawn, drawn, 100.0 * redrawn / drawn, 3e-3 * P * A))
    assert redrawn / drawn <= 3e-5 * P * A
    assert O.gate_margin(X, W, b).min() >= O.GATE


# ---- the layer's host side -------------------------------------------------------------------------------------------------------

def test_constructor_and_shape_errors():
    with pytest.raises(ValueError, match='attention_factor'):
        _layer(0)
    with pytest.raises(TypeError):
        _layer(dropout_rate=0.5)
    with pytest.raises(ValueError, match='same'):
        _layer()([torch.zeros(2, 4), torch.zeros(2, 5)])
    with pytest.raises(ValueError, match='same'):
        _layer()([torch.zeros(2, 4), torch.zeros(3, 4)])
    with pytest.raises(ValueError, match=r'\(B, D\)'):
        _layer()([torch.zeros(2, 4, 1), torch.zeros(2, 4, 1)])
    with pytest.raises(ValueError, match=r'\(B, F, D\)'):
        _layer()(torch.zeros(2, 4))
    with pytest.raises(ValueError, match=r'\(B, F, D\)'):
        _layer()(torch.zeros(2, 4, 3, 1))
    lay = _layer(4)
    lay.build((2, 3, 4))
    with pytest.raises(ValueError, match='attention_W has shape'):
        lay(torch.zeros(2, 3, 5))                          # built for D = 4, called with D = 5
    with pytest.raises(NotImplementedError, match='at most 64 fields'):
        _layer()(torch.zeros(2, 65, 4))
    with pytest.raises(NotImplementedError, match='embedding_dim <= 64'):
        _layer()([torch.zeros(2, 65)] * 2)
    with pytest.raises(NotImplementedError, match='attention_factor <= 64'):
        _layer(65)(torch.zeros(2, 3, 4))


@pytest.mark.parametrize('projection', [True, False])
def test_weight_names_shapes_and_initialisers(projection):
    D, A = 48, 40
    lay = _layer(A, projection=projection)
    lay.build([(3, D)] * 5)
    w = lay.named_weights()
    assert list(w) == ['attention_W', 'attention_b', 'projection_h'] + (['projection_p'] if projection else [])
    shapes = {'attention_W': (D, A), 'attention_b': (A,), 'projection_h': (A, 1), 'projection_p': (D, 1)}
    assert all(tuple(v.shape) == shapes[k] and v.requires_grad for k, v in w.items())
    assert lay.attention_W is w['attention_W'] and (lay.projection_p is w['projection_p'] if projection else lay.projection_p is None)
    assert float(lay.attention_b.detach().abs().max()) == 0.0
    std = (2.0 / (D + A)) ** 0.5                                                # Glorot normal, truncated at two standard deviations
    got = float(lay.attention_W.detach().std())
    assert 0.8 * std <= got <= 1.2 * std and float(lay.attention_W.detach().abs().max()) <= 2 * std / 0.87962566 + 1e-6
    new = np.arange(A, dtype=np.float32)
    lay.set_weights_by_name({'projection_h': new})
    assert np.array_equal(lay.projection_h.detach().numpy()[:, 0], new)
    with pytest.raises(KeyError):
        lay.set_weights_by_name({'kernel': new})
    frozen = _layer(A, trainable=False)
    frozen.build((3, 5, D))
    assert not any(v.requires_grad for v in frozen.named_weights().values())


def test_regularizer_is_kept_with_every_matrix():
    reg = lambda p: (p * p).sum()                                              # noqa: E731
    lay = _layer(2, kernel_initializer=lambda shape: torch.full(tuple(shape), 0.5), kernel_regularizer=reg)
    lay.build((2, 3, 3))
    assert len(lay.losses) == 3 and sorted(float(v.detach()) for v in lay.losses) == pytest.approx([0.5, 0.75, 1.5])


def test_layer_is_exported():
    from rec_now_amd import layers
    from rec_now_amd.layers.afm_layer import AFMLayer
    assert layers.AFMLayer is AFMLayer


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _layer()([torch.zeros(2, 4), torch.zeros(2, 4)])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _layer(projection=False)(torch.zeros(2, 3, 4))


# ---- the library's host-only queries ---------------------------------------------------------------------------------------------

def test_abi_version():
    from rec_now_amd import _lib
    assert _lib.ABI_VERSION >= 27 and _lib.load().recnow_abi_version() >= 27


def test_supported_and_route_queries():
    from rec_now_amd import _lib
    from rec_now_amd.layers.afm_layer import afm_supported
    lib = _lib.load()
    for F in (0, 1, 2, 24, 64, 65):
        for D in (0, 1, 5, 16, 64, 65):
            for A in (0, 1, 4, 7, 64, 65):
                ok = 2 <= F <= 64 and 1 <= D <= 64 and 1 <= A <= 64
                assert lib.recnow_afm_supported(F, D, A) == int(ok), (F, D, A)
                assert afm_supported(F, D, A) == ok
                for bwd in (0, 1):
                    assert lib.recnow_afm_route(F, D, A, bwd) == (0 if ok else -3)      # one route; RECNOW_EUNSUPPORTED
    # entry points refuse what `supported` refuses, before touching any pointer; B = 0 returns without a launch (NULL pointers)
    n = None
    assert lib.recnow_afm_fwd(n, 4, 65, 4, 4, 4, n, n, n, n, n, n) == -3
    assert lib.recnow_afm_fwd(n, 4, 1, 4, 4, 4, n, n, n, n, n, n) == -3                    # a single field has no pair
    assert lib.recnow_afm_bwd(n, 4, n, 4, 4, 4, 4, 65, n, n, n, n, n, n, n, n, n, n, 0, n) == -3
    assert lib.recnow_afm_fwd(n, 4, 4, 4, 4, 0, n, n, n, n, n, n) == -1                    # RECNOW_EINVAL
    assert lib.recnow_afm_fwd(n, 4, 4, 4, 4, 4, n, n, n, n, n, n) == -1                    # NULL pointers with B > 0
    assert lib.recnow_afm_fwd(n, 4, 4, 0, 4, 4, n, n, n, n, n, n) == 0
    assert lib.recnow_afm_bwd(n, 4, n, 4, 4, 0, 4, 4, n, n, n, n, n, n, n, n, n, n, 0, n) == 0


def test_workspace_bytes_follow_the_documented_formula():
    """4 G n rounded up to 256 bytes, n = 4 ceil((D A + 2 A + D) / 4), G = max(1, min(ceil(B / AFM_DW_ROWS), AFM_MAXG, RN_PART_BYTES / (4 n))) --
    read from the constants of csrc/afm.hip.  Bounded by a constant: it does not grow with B or F."""
    from rec_now_amd import _lib
    lib = _lib.load()
    c = _consts()
    rows, maxg = c['AFM_DW_ROWS'], c['AFM_MAXG']
    cap = 32 << 20
    assert '#define RN_PART_BYTES (32u << 20)' in open(os.path.join(ROOT, 'rec_now_amd', 'csrc', 'partials.hpp')).read()
    for B in (0, 1, 3, 4, 5, 4096, 65536, 1 << 20):
        for F in (1, 2, 24, 64, 65):
            for D in (1, 5, 16, 64):
                for A in (1, 4, 7, 64):
                    got = lib.recnow_afm_workspace_bytes(B, F, D, A)
                    if B == 0 or F > 64 or F < 2:
                        assert got == 0
                        continue
                    n = (D * A + 2 * A + D + 3) // 4 * 4
                    G = max(1, min(-(-B // rows), maxg, cap // (4 * n)))
                    assert got == (4 * G * n + 255) // 256 * 256, (B, F, D, A, got)
                    assert got <= cap + 256
                    assert got == lib.recnow_afm_workspace_bytes(B, 2, D, A)         # no F in it
