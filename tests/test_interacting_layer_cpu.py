"""CPU: the fp64 oracle of InteractingLayer is pinned (a hand-worked example, an independent einsum restatement under fp64 autograd, and the
identities of the definition), the input generator's redraw rate is measured, and the host side of the layer is covered: constructor and
shape errors, weight names and shapes, the library's `supported`, `route` and `workspace_bytes` queries, the ABI version, and the refusal
of CPU tensors.

Redraw rate: a sample is redrawn when its smallest |pre| is below 2e-5 of its largest.  For F*E roughly normal values whose largest is about
four standard deviations that happens with probability about F*E * 2 * 2e-5 * 4 * 0.4 = 6.4e-5 F*E: 2.5 % at the benchmark shape (F*E = 384)
and about a quarter at the limit F*E = 4096 (measured: 2.5 %, 8 % at 1280, 23 % at 4096) -- a few percent only up to a few hundred values per
sample.  The redraw leaves no entry out of any comparison; it only costs draws."""
import os
import re

import numpy as np
import pytest
import torch

import _autoint_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layer(*a, **k):
    from rec_now_amd.layers.interacting_layer import InteractingLayer
    return InteractingLayer(*a, **k)


def _consts():
    src = open(os.path.join(ROOT, 'rec_now_amd', 'csrc', 'autoint.hip')).read()
    return {k: int(v) for k, v in re.findall(r'#define (AI_[A-Z_]+) \(?(\d+)\)?\s', src)}


# ---- the oracle ------------------------------------------------------------------------------------------------------------------

def test_oracle_matches_a_hand_worked_example():
    """F = 2, D = 2, H = 1, d = 1: x0 = (1, 0), x1 = (0, 1); Wq = (ln 2, 0)^T, Wk = (1, 0)^T, Wv = (2, 4)^T, Wr = (-3, 1)^T.
    q = (ln 2, 0), k = (1, 0), v = (2, 4).  Query 0: s = (ln 2, 0), a = (2/3, 1/3), o = 8/3, pre = 8/3 - 3 = -1/3 -> relu 0.
    Query 1: s = (0, 0), a = (1/2, 1/2), o = 3, pre = 4."""
    X = np.array([[[1., 0.], [0., 1.]]])
    Wq, Wk, Wv, Wr = np.array([[np.log(2.)], [0.]]), np.array([[1.], [0.]]), np.array([[2.], [4.]]), np.array([[-3.], [1.]])
    r = O.run(X, Wq, Wk, Wv, Wr, 1, 1, g=np.array([[[5.], [1.]]]))
    assert np.allclose(r['pre'][0, :, 0], [-1. / 3, 4.], rtol=0, atol=1e-15) and r['out'][0, :, 0].tolist() == [0., r['pre'][0, 1, 0]]
    assert r['ratio'][0] == pytest.approx(1. / 12)
    # backward: dpre = (0, 1) (query 0 is cut by the ReLU).  Query 1: dA = (2, 4), rd = 3, dS = (1/2)(−1, 1); dV = (1/2, 1/2);
    # dQ_1 = dS . k = −1/2;  dK = dS * q_1 = 0.   dX_0 = dV_0 Wv^T = (1, 2);  dX_1 = dQ_1 Wq^T + dV_1 Wv^T + dpre_1 Wr^T
    assert np.allclose(r['dX'][0, 0], [1., 2.], atol=1e-15)
    assert np.allclose(r['dX'][0, 1], [-0.5 * np.log(2.) + 1. - 3., 0. + 2. + 1.], atol=1e-15)
    assert np.allclose(r['dWv'][:, 0], [0.5, 0.5], atol=1e-15) and np.allclose(r['dWr'][:, 0], [0., 1.], atol=1e-15)
    assert np.allclose(r['dWq'][:, 0], [0., -0.5], atol=1e-15) and np.allclose(r['dWk'][:, 0], [0., 0.], atol=1e-15)


def _compose(X, Wq, Wk, Wv, Wr, H, d, scaling, relu):
    B, F, _ = X.shape
    Q, K, V = ((X @ W).reshape(B, F, H, d) for W in (Wq, Wk, Wv))
    S = torch.einsum('bihc,bjhc->bhij', Q, K)
    if scaling:
        S = S / d ** 0.5
    out = torch.einsum('bhij,bjhc->bihc', torch.softmax(S, -1), V).reshape(B, F, H * d)
    if Wr is not None:
        out = out + X @ Wr
    return torch.relu(out) if relu else out


@pytest.mark.parametrize('use_res,scaling,relu', [(True, False, True), (False, True, True), (True, True, False), (False, False, False)])
def test_oracle_matches_fp64_autograd_of_an_einsum_restatement(use_res, scaling, relu):
    B, F, D, H, d = 6, 5, 7, 3, 2
    X, Wq, Wk, Wv, Wr, g = O.draw(np.random.default_rng(3), B, F, D, H, d, use_res, scaling)
    r = O.run(X, Wq, Wk, Wv, Wr, H, d, scaling, relu, g)
    t = [torch.tensor(a, dtype=torch.float64, requires_grad=True) if a is not None else None for a in (X, Wq, Wk, Wv, Wr)]
    out = _compose(*t, H, d, scaling, relu)
    leaves = [a for a in t if a is not None]
    grads = torch.autograd.grad(out, leaves, torch.tensor(g, dtype=torch.float64))
    assert O.reltensor(r['out'], out.detach().numpy()) <= 1e-12
    assert O.reltensor(r['pre'], O.pre_einsum(X, Wq, Wk, Wv, Wr, H, d, scaling)) <= 1e-12
    for name, got in zip(['dX', 'dWq', 'dWk', 'dWv'] + (['dWr'] if use_res else []), grads):
        assert O.reltensor(r[name], got.numpy()) <= 1e-12, name
    assert use_res or r['dWr'] is None


def test_zero_query_weights_give_uniform_attention():
    X, Wq, Wk, Wv, Wr, _ = O.draw(np.random.default_rng(4), 5, 6, 4, 2, 3)
    r = O.run(X, np.zeros_like(Wq), Wk, Wv, Wr, 2, 3, relu=False)
    X64 = X.astype(np.float64)
    want = (X64 @ Wv).mean(1, keepdims=True) + X64 @ Wr
    assert np.abs(r['pre'] - want).max() <= 1e-13


def test_single_field_is_a_dense_layer():
    X, Wq, Wk, Wv, Wr, _ = O.draw(np.random.default_rng(5), 7, 1, 5, 2, 2)
    r = O.run(X, Wq, Wk, Wv, Wr, 2, 2)
    want = np.maximum(X.astype(np.float64)[:, 0] @ (Wv.astype(np.float64) + Wr), 0.0)
    assert np.abs(r['out'][:, 0] - want).max() <= 1e-13


def test_permuting_the_fields_permutes_the_output_blocks():
    X, Wq, Wk, Wv, Wr, g = O.draw(np.random.default_rng(6), 4, 6, 5, 2, 3)
    perm = np.array([3, 0, 5, 1, 4, 2])
    a, b = O.run(X, Wq, Wk, Wv, Wr, 2, 3, g=g), O.run(X[:, perm], Wq, Wk, Wv, Wr, 2, 3, g=g[:, perm])
    assert np.abs(a['out'][:, perm] - b['out']).max() <= 1e-13 and np.abs(a['dX'][:, perm] - b['dX']).max() <= 1e-12
    assert np.abs(a['dWq'] - b['dWq']).max() <= 1e-12


def test_heads_are_independent_one_head_layers():
    H, d = 3, 2
    X, Wq, Wk, Wv, Wr, _ = O.draw(np.random.default_rng(7), 4, 5, 6, H, d)
    whole = O.run(X, Wq, Wk, Wv, Wr, H, d)['out']
    for h in range(H):
        hs = slice(h * d, (h + 1) * d)
        one = O.run(X, Wq[:, hs], Wk[:, hs], Wv[:, hs], Wr[:, hs], 1, d)['out']
        assert np.array_equal(one, whole[:, :, hs])


def test_scaling_equals_scaled_query_weights():
    X, Wq, Wk, Wv, Wr, g = O.draw(np.random.default_rng(8), 4, 5, 6, 2, 4)
    a = O.run(X, Wq, Wk, Wv, Wr, 2, 4, scaling=True, g=g)
    b = O.run(X, Wq.astype(np.float64) / 2.0, Wk, Wv, Wr, 2, 4, scaling=False, g=g)
    assert np.abs(a['out'] - b['out']).max() <= 1e-13 and np.abs(a['dX'] - b['dX']).max() <= 1e-12
    assert np.abs(a['dWq'] - b['dWq'] / 2.0).max() <= 1e-12          # the chain rule through W_query / sqrt(d)


def test_kink_ratio_and_relrow():
    pre = np.array([[[4., -1.], [2., 8.]], [[0., 0.], [0., 0.]]])
    assert O.kink_ratio(pre).tolist() == [0.125, 1.0]
    ref = np.array([[1., 0.], [1000., 0.]])
    assert O.relrow(ref + np.array([[0., 0.], [0., 1.]]), ref) == pytest.approx(1e-3)
    assert O.relrow(np.full((2, 2), np.nan), ref) == float('inf')


@pytest.mark.parametrize('B,F,D,H,d,most', [(2000, 24, 16, 2, 8, 0.05), (1500, 8, 16, 2, 8, 0.02), (300, 64, 64, 8, 8, 0.35)])
def test_redraw_rate(B, F, D, H, d, most):
    """A few percent per sample up to a few hundred values per sample; at the limit F*E = 4096 about a quarter (see the docstring of the file).
    Held to twice the estimate 6.4e-5 F*E."""
    count = []
    X, Wq, Wk, Wv, Wr, _ = O.draw(np.random.default_rng(1), B, F, D, H, d, count=count)
    redrawn, drawn = count[0]
    print('F*E %d: %d of %d samples redrawn (%.1f %%)' % (F * H * d, redrawn, drawn, 100.0 * redrawn / drawn))
    assert redrawn / drawn <= most and redrawn / drawn <= 2 * 6.4e-5 * F * H * d
    assert O.kink_ratio(O.pre_einsum(X, Wq, Wk, Wv, Wr, H, d)).min() >= O.KINK


# ---- the layer's host side -------------------------------------------------------------------------------------------------------

def test_constructor_and_shape_errors():
    with pytest.raises(ValueError, match='head_num'):
        _layer(8, 0)
    with pytest.raises(ValueError, match='att_embedding_size'):
        _layer(0, 2)
    with pytest.raises(ValueError, match='activation'):
        _layer(activation='tanh')
    with pytest.raises(TypeError):
        _layer(units=3)
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
    lay = _layer(4, 2)
    lay.build((2, 3, 4))
    with pytest.raises(ValueError, match='W_query has shape'):
        lay(torch.zeros(2, 3, 5))                          # built for D = 4, called with D = 5
    with pytest.raises(NotImplementedError, match='at most 64 fields'):
        _layer()(torch.zeros(2, 65, 4))
    with pytest.raises(NotImplementedError, match='embedding_dim <= 64'):
        _layer()([torch.zeros(2, 65)] * 2)
    with pytest.raises(NotImplementedError, match='<= 64'):
        _layer(13, 5)(torch.zeros(2, 3, 4))                # E = 65
    with pytest.raises(NotImplementedError, match='head_num <= 8'):
        _layer(1, 9)(torch.zeros(2, 3, 4))


@pytest.mark.parametrize('use_res', [True, False])
def test_weight_names_and_shapes(use_res):
    D, H, d = 6, 3, 4
    lay = _layer(d, H, use_res=use_res)
    lay.build([(3, D)] * 5)
    w = lay.named_weights()
    assert list(w) == ['W_query', 'W_key', 'W_value'] + (['W_res'] if use_res else [])
    assert all(tuple(v.shape) == (D, H * d) and v.requires_grad for v in w.values())
    assert w['W_query'] is lay.W_query and w['W_value'] is lay.W_value and (lay.W_res is w['W_res'] if use_res else lay.W_res is None)
    limit = (6.0 / (D + H * d)) ** 0.5                                          # Glorot fans of ONE (D, E) matrix
    assert all(float(v.detach().abs().max()) <= limit + 1e-6 for v in w.values())
    assert float(lay.W_query.detach().abs().max()) > 0.5 * limit
    new = np.arange(D * H * d, dtype=np.float32).reshape(D, H * d)
    lay.set_weights_by_name({'W_key': new})
    assert np.array_equal(lay.W_key.detach().numpy(), new)
    with pytest.raises(KeyError):
        lay.set_weights_by_name({'kernel': new})
    frozen = _layer(d, H, trainable=False)
    frozen.build((3, 5, D))
    assert not any(v.requires_grad for v in frozen.named_weights().values())


def test_regularizer_is_kept_with_every_weight():
    reg = lambda p: (p * p).sum()                                              # noqa: E731
    lay = _layer(2, 2, kernel_initializer=lambda shape: torch.full(tuple(shape), 0.5), kernel_regularizer=reg)
    lay.build((2, 3, 3))
    assert len(lay.losses) == 4 and all(float(v) == pytest.approx(0.25 * 12) for v in lay.losses)


def test_layer_is_exported():
    from rec_now_amd import layers
    from rec_now_amd.layers.interacting_layer import InteractingLayer
    assert layers.InteractingLayer is InteractingLayer


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _layer()([torch.zeros(2, 4), torch.zeros(2, 4)])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _layer()(torch.zeros(2, 3, 4))


# ---- the library's host-only queries ---------------------------------------------------------------------------------------------

def test_abi_version():
    from rec_now_amd import _lib
    assert _lib.ABI_VERSION >= 26 and _lib.load().recnow_abi_version() >= 26


def test_supported_and_route_queries():
    from rec_now_amd import _lib
    from rec_now_amd.layers.interacting_layer import autoint_supported
    lib = _lib.load()
    for F in (0, 1, 24, 64, 65):
        for D in (0, 1, 5, 16, 64, 65):
            for H, d in ((1, 1), (2, 8), (8, 8), (8, 9), (9, 1), (1, 64), (1, 65), (0, 4), (2, 0)):
                ok = 1 <= F <= 64 and 1 <= D <= 64 and 1 <= H <= 8 and d >= 1 and H * d <= 64
                assert lib.recnow_autoint_supported(F, D, H, d) == int(ok), (F, D, H, d)
                assert autoint_supported(F, D, H, d) == ok
                for bwd in (0, 1):
                    for res in (0, 1):
                        route = lib.recnow_autoint_route(F, D, H, d, res, bwd)
                        assert (route in (0, 1)) if ok else route == -3         # RECNOW_EUNSUPPORTED
    # 4 KB of weights are resident; at the limits three or four 64 x 64 matrices beside the tiles of 64 fields are not
    assert lib.recnow_autoint_route(24, 16, 2, 8, 1, 0) == 0 and lib.recnow_autoint_route(24, 16, 2, 8, 1, 1) == 0
    assert lib.recnow_autoint_route(64, 64, 8, 8, 1, 1) == 1 and lib.recnow_autoint_route(40, 64, 8, 8, 1, 0) == 1
    # entry points refuse what `supported` refuses, before touching any pointer; B = 0 returns without a launch (NULL pointers)
    n = None
    assert lib.recnow_autoint_fwd(n, 4, 65, 4, 4, 1, 4, n, n, n, n, 0, 1, n, n) == -3
    assert lib.recnow_autoint_fwd(n, 4, 4, 4, 4, 9, 4, n, n, n, n, 0, 1, n, n) == -3
    assert lib.recnow_autoint_bwd(n, 4, n, 4, 4, 4, 65, 1, 4, n, n, n, n, 0, 1, n, n, n, n, n, n, 0, n) == -3
    assert lib.recnow_autoint_fwd(n, 4, 4, 4, 4, 0, 4, n, n, n, n, 0, 1, n, n) == -1          # RECNOW_EINVAL
    assert lib.recnow_autoint_fwd(n, 4, 4, 4, 4, 1, 4, n, n, n, n, 0, 1, n, n) == -1          # NULL pointers with B > 0
    assert lib.recnow_autoint_fwd(n, 4, 4, 0, 4, 1, 4, n, n, n, n, 0, 1, n, n) == 0
    assert lib.recnow_autoint_bwd(n, 4, n, 4, 4, 0, 4, 1, 4, n, n, n, n, 0, 1, n, n, n, n, n, n, 0, n) == 0


def test_workspace_bytes_follow_the_documented_formula():
    """4 G nW D E rounded up to 256 bytes, nW = 3 + use_res, G = max(1, min(ceil(B / AI_DW_ROWS), AI_MAXG, RN_PART_BYTES / (4 nW D E))) --
    read from the constants of csrc/autoint.hip.  Bounded by a constant: it does not grow as B F."""
    from rec_now_amd import _lib
    lib = _lib.load()
    c = _consts()
    rows, maxg = c['AI_DW_ROWS'], c['AI_MAXG']
    cap = 32 << 20
    assert '#define RN_PART_BYTES (32u << 20)' in open(os.path.join(ROOT, 'rec_now_amd', 'csrc', 'partials.hpp')).read()
    for B in (0, 1, 7, 8, 9, 4096, 65536, 1 << 20):
        for F in (1, 24, 64, 65):
            for D in (1, 5, 16, 64):
                for H, d in ((1, 1), (2, 8), (7, 9), (8, 8)):
                    for res in (0, 1):
                        got = lib.recnow_autoint_workspace_bytes(B, F, D, H, d, res)
                        if B == 0 or F > 64:
                            assert got == 0
                            continue
                        nW, E = 3 + res, H * d
                        G = max(1, min(-(-B // rows), maxg, cap // (4 * nW * D * E)))
                        assert got == (4 * G * nW * D * E + 255) // 256 * 256, (B, F, D, H, d, res, got)
                        assert got <= max(cap, 4 * nW * D * E) + 256
                        assert got == lib.recnow_autoint_workspace_bytes(B, 1, D, H, d, res)     # no F in it
