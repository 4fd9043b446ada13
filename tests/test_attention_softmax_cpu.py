"""CPU: the fp64 oracle of attention_by_softmax and TargetAttentionLayer (tests/_attention_softmax_oracle.py) is pinned -- a hand-worked
example, fp64 torch autograd of the masked_fill + softmax composition, the invariances of the definition, the folded form of the layer -- and
the host side is covered: argument errors, both refusals, empty shapes without a library call, the ABI version, the library's `supported`,
`route` and `tile` queries and the C entries' argument checks.  The last test holds the plain fp32 torch composition on the CPU under half of
every bound of tests/test_attention_softmax_gpu.py on every shape and mode of that file, so those bounds leave room for an fp32 kernel."""
import math

import numpy as np
import pytest
import torch

import _attention_softmax_oracle as O


def _tile():
    from rec_now_amd import _lib
    lib = _lib.load()
    return tuple(lib.recnow_attention_softmax_tile(i) for i in range(3))


def _compose(x, q, key, scale):
    """einsum + masked_fill + softmax + einsum, with the empty-row patch; x (B, L, D), q (B, H, D), key (B, L) bool."""
    s = torch.einsum('bhd,bld->bhl', q, x) * scale
    s = s.masked_fill(~key[:, None, :], float('-inf'))
    a = torch.softmax(s, -1)
    a = torch.where(key.any(1)[:, None, None], a, torch.zeros_like(a))
    return torch.einsum('bhl,bld->bhd', a, x)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

def test_oracle_matches_a_hand_worked_example():
    """B = 1, L = 3, D = 2, H = 1, scale 1, position 1 masked: x = ((ln 2, 0), (5, 5), (0, 1)), q = (1, 0).
    s = (ln 2, -, 0);  a = (2/3, 0, 1/3);  out = (2/3 ln 2, 1/3);  lse = ln 3.
    dc = (3, 0): g = (3 ln 2, -, 0), gbar = 2 ln 2, ds = (2/3 ln 2, 0, -2/3 ln 2);
    dx_0 = 2/3 (3, 0) + ds_0 (1, 0),  dx_1 = 0,  dx_2 = 1/3 (3, 0) + ds_2 (1, 0);  dq = ds_0 x_0 + ds_2 x_2 = (2/3 ln^2 2, -2/3 ln 2)."""
    ln2 = math.log(2.0)
    x = np.array([[[ln2, 0.], [5., 5.], [0., 1.]]])
    q, dc = np.array([[[1., 0.]]]), np.array([[[3., 0.]]])
    r = O.run(x, q, mask=np.array([[1, 0, 1]]), scale=1.0, dc=dc)
    assert np.allclose(r['a'][0, 0], [2. / 3, 0., 1. / 3], rtol=0, atol=1e-15)
    assert np.allclose(r['out'][0, 0], [2. / 3 * ln2, 1. / 3], rtol=0, atol=1e-15) and r['lse'][0, 0] == pytest.approx(math.log(3.0), abs=1e-15)
    assert np.allclose(r['ds'][0, 0], [2. / 3 * ln2, 0., -2. / 3 * ln2], rtol=0, atol=1e-15)
    assert np.allclose(r['dx'][0], [[2. + 2. / 3 * ln2, 0.], [0., 0.], [1. - 2. / 3 * ln2, 0.]], rtol=0, atol=1e-15)
    assert np.allclose(r['dq'][0, 0], [2. / 3 * ln2 * ln2, -2. / 3 * ln2], rtol=0, atol=1e-15)
    same = O.run(x, q, lengths=np.array([3]), mask=np.array([[1, 0, 1]]), scale=1.0, dc=dc)
    assert all(np.array_equal(r[k], same[k]) for k in r)


@pytest.mark.parametrize('mode', O.MODES)
def test_oracle_matches_fp64_autograd_of_the_composition(mode):
    B, L, D, H = 6, 9, 5, 3
    x, q, dc, lengths, mask = O.draw(np.random.default_rng(11), B, L, D, H, mode)
    r = O.run(x, q, lengths, mask, 0.37, dc)
    key = torch.from_numpy(r['key'])
    xt, qt = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (x, q))
    out = _compose(xt, qt, key, 0.37)
    dx, dq = torch.autograd.grad(out, (xt, qt), torch.tensor(dc, dtype=torch.float64))
    has = r['key'].any(1)
    assert has[0] and (mode == 'none' or not has[-1])
    for name, got in (('out', out.detach()), ('dx', dx), ('dq', dq)):
        assert np.abs(r[name][has] - got.numpy()[has]).max() <= 1e-12, name
        assert not r[name][~has].any(), name                               # a sample without a key: exactly zero everywhere
    s = torch.einsum('bhd,bld->bhl', qt, xt).detach() * 0.37
    lse = torch.logsumexp(s.masked_fill(~key[:, None, :], float('-inf')), -1).numpy()
    assert np.abs(r['lse'][has] - lse[has]).max() <= 1e-12 and np.isneginf(r['lse'][~has]).all()


def _inv_case(seed=5, B=4, L=7, D=3, H=2):
    return O.draw(np.random.default_rng(seed), B, L, D, H, 'both')


def test_lengths_equal_the_equivalent_mask():
    x, q, dc, lengths, _ = _inv_case()
    a = O.run(x, q, lengths=lengths, dc=dc)
    b = O.run(x, q, mask=(np.arange(x.shape[1])[None, :] < lengths[:, None]).astype(np.float32), dc=dc)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    big = O.run(x, q, lengths=np.where(lengths == x.shape[1], 10 ** 12, np.where(lengths == 0, -3, lengths)), dc=dc)
    assert all(np.array_equal(a[k], big[k]) for k in a)                     # above L acts as L, negative as 0


def test_heads_equal_separate_one_head_calls():
    x, q, dc, lengths, mask = _inv_case()
    r = O.run(x, q, lengths, mask, dc=dc)
    dx = np.zeros_like(r['dx'])
    for h in range(q.shape[1]):
        one = O.run(x, q[:, h:h + 1], lengths, mask, dc=dc[:, h:h + 1])
        assert np.array_equal(one['out'][:, 0], r['out'][:, h]) and np.array_equal(one['dq'][:, 0], r['dq'][:, h])
        assert np.array_equal(one['lse'][:, 0], r['lse'][:, h])
        dx += one['dx']
    assert np.abs(dx - r['dx']).max() <= 1e-14


def test_scale_equals_a_scaled_query():
    x, q, dc, lengths, mask = _inv_case()
    a = O.run(x, q, lengths, mask, 0.25, dc)                                # a power of two: q * 0.25 is exact
    b = O.run(x, q.astype(np.float64) * 0.25, lengths, mask, 1.0, dc)
    assert np.abs(a['out'] - b['out']).max() <= 1e-14 and np.abs(a['dx'] - b['dx']).max() <= 1e-14
    assert np.abs(a['dq'] - 0.25 * b['dq']).max() <= 1e-14                  # d / dq = 0.25 d / d(0.25 q)


def test_a_permutation_of_the_positions_changes_nothing():
    x, q, dc, lengths, mask = _inv_case()
    key = O.keys_of(*x.shape[:2], lengths, mask)
    perm = np.array([3, 0, 6, 1, 5, 2, 4])
    a, b = O.run(x, q, mask=key, dc=dc), O.run(x[:, perm], q, mask=key[:, perm], dc=dc)
    assert np.abs(a['out'] - b['out']).max() <= 1e-14 and np.abs(a['lse'][key.any(1)] - b['lse'][key.any(1)]).max() <= 1e-14
    assert np.abs(a['dx'][:, perm] - b['dx']).max() <= 1e-14 and np.abs(a['dq'] - b['dq']).max() <= 1e-14


def test_adding_masked_positions_changes_nothing():
    x, q, dc, lengths, mask = _inv_case()
    key = O.keys_of(*x.shape[:2], lengths, mask)
    junk = np.full((x.shape[0], 3, x.shape[2]), np.nan, dtype=np.float32)
    a = O.run(x, q, mask=key, dc=dc)
    b = O.run(np.concatenate([x, junk], 1), q, mask=np.concatenate([key, np.zeros((x.shape[0], 3), dtype=bool)], 1), dc=dc)
    assert np.array_equal(a['out'], b['out']) and np.array_equal(a['dq'], b['dq']) and np.array_equal(a['lse'], b['lse'])
    assert np.array_equal(a['dx'], b['dx'][:, :x.shape[1]]) and not b['dx'][:, x.shape[1]:].any()


def test_the_weights_sum_to_one_and_the_score_gradients_to_zero():
    x, q, dc, lengths, mask = _inv_case()
    r = O.run(x, q, lengths, mask, dc=dc)
    has = r['key'].any(1)
    assert np.abs(r['a'][has].sum(-1) - 1.0).max() <= 1e-15 and not r['a'][~has].any()
    assert np.abs(r['ds'].sum(-1)).max() <= 1e-14 and not r['a'][~np.broadcast_to(r['key'][:, None, :], r['a'].shape)].any()


@pytest.mark.parametrize('scaling', [True, False])
def test_the_folded_layer_equals_its_unfolded_definition(scaling):
    """k~ = W_key,h Q_h into the op, the pooled context through W_value,h: the form layers/target_attention_layer.py runs, in fp64."""
    rng = np.random.default_rng(8)
    B, L, D, Dq, H, d = 5, 6, 4, 3, 2, 3
    x, doc, g = rng.standard_normal((B, L, D)), rng.standard_normal((B, Dq)), rng.standard_normal((B, H * d))
    Wq, Wk, Wv = rng.standard_normal((Dq, H * d)), rng.standard_normal((D, H * d)), rng.standard_normal((D, H * d))
    lengths = np.array([6, 0, 3, 1, 5])
    ref = O.run_layer(x, doc, Wq, Wk, Wv, H, scaling, lengths=lengths, g=g)
    Q = (doc @ Wq).reshape(B, H, d)
    folded = np.stack([np.stack([Wk[:, h * d:(h + 1) * d] @ Q[b, h] for h in range(H)]) for b in range(B)])
    Wv3 = Wv.reshape(D, H, d)
    dc = np.stack([np.stack([Wv3[:, h] @ g[b, h * d:(h + 1) * d] for h in range(H)]) for b in range(B)])
    r = O.run(x, folded, lengths=lengths, scale=1.0 / math.sqrt(d) if scaling else 1.0, dc=dc)
    out = np.stack([np.concatenate([r['out'][b, h] @ Wv3[:, h] for h in range(H)]) for b in range(B)])
    assert np.abs(out - ref['out']).max() <= 1e-12 and not ref['out'][1].any()
    assert np.abs(r['dx'] - ref['dx']).max() <= 1e-12 and not ref['dx'][1].any()
    dWq, dWk, dWv, ddoc = np.zeros_like(Wq), np.zeros_like(Wk), np.zeros_like(Wv), np.zeros_like(doc)
    for b in range(B):
        for h in range(H):
            cols = slice(h * d, (h + 1) * d)
            dQ = Wk[:, cols].T @ r['dq'][b, h]                              # k~ = W_key,h Q_h
            dWv[:, cols] += np.outer(r['out'][b, h], g[b, cols])
            dWk[:, cols] += np.outer(r['dq'][b, h], Q[b, h])
            dWq[:, cols] += np.outer(doc[b], dQ)
            ddoc[b] += Wq[:, cols] @ dQ
    for name, got in (('dWq', dWq), ('dWk', dWk), ('dWv', dWv), ('ddoc', ddoc)):
        assert np.abs(got - ref[name]).max() <= 1e-12, name


# ---- the host side -------------------------------------------------------------------------------------------------------------------

def _op(*a, **k):
    from rec_now_amd.rec_block.attention import attention_by_softmax
    return attention_by_softmax(*a, **k)


def test_argument_errors():
    x, q = torch.zeros(4, 5, 8), torch.zeros(4, 2, 8)
    for bad_x, bad_q in ((torch.zeros(4, 8), q), (x, torch.zeros(8)), (x, torch.zeros(4, 2, 8, 1)), (x, torch.zeros(3, 2, 8)), (x, torch.zeros(4, 2, 7)),
                         (x, torch.zeros(4, 7))):
        with pytest.raises(ValueError, match=r'\(B, L, D\)'):
            _op(bad_x, bad_q)
    with pytest.raises(ValueError, match='integers'):
        _op(x, q, lengths=torch.zeros(4))
    for n in (torch.zeros(3, dtype=torch.int64), torch.zeros(4, 2, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)):
        with pytest.raises(ValueError, match='lengths must be'):
            _op(x, q, lengths=n)
    for m in (torch.zeros(4, 4), torch.zeros(20), torch.zeros(5, 4), torch.zeros(4, 5, 1)):
        with pytest.raises(ValueError, match='mask must be'):
            _op(x, q, mask=m)
    for s in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='scale'):
            _op(x, q, scale=s)
    with pytest.raises(TypeError):
        _op(x.numpy(), q)


def test_refusals_come_after_the_argument_checks_and_before_the_device():
    with pytest.raises(NotImplementedError, match='embedding_dim <= 256'):
        _op(torch.zeros(2, 3, 257), torch.zeros(2, 257))
    with pytest.raises(NotImplementedError, match='at most 8 heads'):
        _op(torch.zeros(2, 3, 4), torch.zeros(2, 9, 4))
    with pytest.raises(ValueError, match='scale'):
        _op(torch.zeros(2, 3, 257), torch.zeros(2, 257), scale=0.0)
    for args in ((torch.zeros(2, 3, 4), torch.zeros(2, 4)), (torch.zeros(2, 3, 256), torch.zeros(2, 8, 256))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            _op(*args)


def test_empty_shapes_make_no_library_call(monkeypatch):
    """B = 0 and L = 0 return without a launch: zeros and lse = -inf, zero gradients.  (The device check is lifted for this test only.)"""
    from rec_now_amd import _lib

    def refuse(*a):
        raise AssertionError('library call on an empty shape: %r' % (a[0],))
    monkeypatch.setattr(_lib, 'require_gpu', lambda t, what='tensor': t)
    monkeypatch.setattr(_lib, 'call', refuse)
    for B, L, H in ((0, 5, 2), (3, 0, 2), (0, 0, 1)):
        x = torch.zeros(B, L, 4, requires_grad=True)
        q = torch.ones(B, H, 4, requires_grad=True)
        out, lse = _op(x, q, lengths=torch.zeros(B, dtype=torch.int64), mask=torch.ones(B, L), return_lse=True)
        assert out.shape == (B, H, 4) and lse.shape == (B, H) and not out.any() and bool(torch.isneginf(lse).all())
        assert not lse.requires_grad
        out.sum().backward()
        assert x.grad.shape == x.shape and not x.grad.any() and not q.grad.any()
    out, lse = _op(torch.zeros(3, 0, 4), torch.ones(3, 4), return_lse=True)
    assert out.shape == (3, 4) and lse.shape == (3,)


def test_layer_host_side():
    from rec_now_amd import layers
    from rec_now_amd.layers.target_attention_layer import TargetAttentionLayer
    assert layers.TargetAttentionLayer is TargetAttentionLayer
    for kw in (dict(head_num=0), dict(att_embedding_size=0)):
        with pytest.raises(ValueError):
            TargetAttentionLayer(**kw)
    with pytest.raises(TypeError):
        TargetAttentionLayer(dropout_rate=0.1)
    lay = TargetAttentionLayer(3, 5)
    with pytest.raises(ValueError, match=r'\(B, L, D\)'):
        lay(torch.zeros(2, 4), torch.zeros(2, 4))
    with pytest.raises(ValueError, match=r'\(B, L, D\)'):
        lay(torch.zeros(2, 3, 4), torch.zeros(3, 6))
    lay.build(((2, 7, 4), (2, 6)))
    w = lay.named_weights()
    assert list(w) == ['W_query', 'W_key', 'W_value'] and [tuple(v.shape) for v in w.values()] == [(6, 15), (4, 15), (4, 15)]
    lim = math.sqrt(6.0 / (4 + 15))
    assert float(lay.W_key.detach().abs().max()) <= lim and all(v.requires_grad for v in w.values())
    with pytest.raises(ValueError, match='W_key has shape'):
        lay(torch.zeros(2, 7, 5), torch.zeros(2, 6))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        lay(torch.zeros(2, 7, 4), torch.zeros(2, 6))
    with pytest.raises(NotImplementedError, match='at most 8 heads'):
        TargetAttentionLayer(9, 2)(torch.zeros(2, 7, 4), torch.zeros(2, 6))
    frozen = TargetAttentionLayer(trainable=False)
    frozen.build(((2, 7, 4), (2, 6)))
    assert not any(v.requires_grad for v in frozen.named_weights().values())


# ---- the library's host-only queries -------------------------------------------------------------------------------------------------

def test_abi_version():
    from rec_now_amd import _lib
    assert _lib.ABI_VERSION >= 34 and _lib.load().recnow_abi_version() >= 34


def _route(D, H, mis):
    hb = 1 if H <= 1 else 2 if H <= 2 else 4 if H <= 4 else 8
    if D % 4 == 0 and D // 4 in (1, 2, 4, 8, 16) and not mis:
        return 200000 + 100 * (D // 4) + hb
    return 100000 + 100 * (16 if D <= 16 else 32 if D <= 32 else 64) + hb


def test_supported_route_and_tile_queries():
    from rec_now_amd import _lib
    from rec_now_amd.rec_block.attention import attention_softmax_supported
    lib = _lib.load()
    spw, trip, lanes = _tile()
    assert spw * lanes == 64 and trip % lanes == 0 and trip // lanes >= 1          # a wave of `spw` samples, whole pieces per lane
    assert lib.recnow_attention_softmax_tile(3) == -1 and lib.recnow_attention_softmax_tile(-1) == -1
    for L in (-1, 0, 1, 200):
        for D in (0, 1, 3, 4, 20, 64, 256, 257):
            for H in (0, 1, 3, 8, 9):
                ok = L >= 0 and 1 <= D <= 256 and 1 <= H <= 8
                assert lib.recnow_attention_softmax_supported(L, D, H) == int(ok) and attention_softmax_supported(L, D, H) == ok
                for which, top in ((0, 7), (1, 63)):
                    want = -1 if (L < 0 or D < 1 or H < 1) else -3 if not ok else None
                    for mis in (0, 1, top):
                        got = lib.recnow_attention_softmax_route(which, 5, L, D, H, mis)
                        assert got == (_route(D, H, mis) if want is None else want), (which, L, D, H, mis)
    assert lib.recnow_attention_softmax_route(0, 0, 3, 16, 2, 0) == 0                # B = 0: nothing is launched
    for bad in ((2, 5, 3, 16, 2, 0), (-1, 5, 3, 16, 2, 0), (0, -1, 3, 16, 2, 0), (0, 5, 3, 16, 2, 8), (1, 5, 3, 16, 2, 64), (0, 5, 3, 16, 2, -1)):
        assert lib.recnow_attention_softmax_route(*bad) == -1, bad
    # every instantiation has a shape in the GPU file
    seen = {lib.recnow_attention_softmax_route(w, B, L, D, H, 0) // 100 for (B, L, D, H) in O.shapes(spw, trip, lanes) for w in (0, 1)}
    assert seen == {2001, 2002, 2004, 2008, 2016, 1016, 1032, 1064}


def test_c_entries_check_their_arguments():
    """Refusals come before any pointer is touched (NULL everywhere); B = 0 returns OK without a launch."""
    from rec_now_amd import _lib
    lib = _lib.load()
    n = None
    fwd = lambda B, L, D, H, s=1.0: lib.recnow_attention_softmax_fwd(n, n, n, n, B, L, D, H, s, n, n, n)             # noqa: E731
    bwd = lambda B, L, D, H, s=1.0: lib.recnow_attention_softmax_bwd(n, n, n, n, n, n, n, B, L, D, H, s, n, n, n)    # noqa: E731
    for f in (fwd, bwd):
        assert f(-1, 3, 4, 1) == -1 and f(2, -1, 4, 1) == -1 and f(2, 3, 0, 1) == -1 and f(2, 3, 4, 0) == -1
        assert f(2, 3, 257, 1) == -3 and f(2, 3, 4, 9) == -3
        for s in (0.0, -1.0, float('inf'), float('nan')):
            assert f(2, 3, 4, 1, s) == -1
        assert f(0, 3, 4, 1) == 0 and f(0, 0, 256, 8) == 0
        assert f(2, 3, 4, 1) == -1                                           # NULL pointers with B > 0


# ---- the bounds of the GPU file ------------------------------------------------------------------------------------------------------

def test_fp32_composition_stays_under_half_of_every_gpu_bound():
    """Plain fp32 torch (einsum, masked_fill, softmax, einsum) on the CPU, on every shape and mode of the GPU file, against the bounds that file
    uses: per row 1e-5 max(1, max |ref row|) for out, dx (a row is a position) and dquery, 1e-6 max(1, |lse|) for lse."""
    spw, trip, lanes = _tile()
    worst = {}
    for shape in O.shapes(spw, trip, lanes):
        for mode in O.MODES:
            c = O.case(*shape, mode)
            key = torch.from_numpy(c['ref']['key'].copy())
            x, q = (torch.tensor(c[k], requires_grad=True) for k in ('x', 'q'))
            scale = 1.0 / math.sqrt(shape[2])
            out = _compose(x, q, key, scale)
            dx, dq = torch.autograd.grad(out, (x, q), torch.tensor(c['dc']))
            s = (torch.einsum('bhd,bld->bhl', q, x).detach() * scale).masked_fill(~key[:, None, :], float('-inf'))
            got = dict(out=out.detach().numpy(), dx=dx.numpy(), dq=dq.numpy())
            has = c['ref']['key'].any(1)
            for k, v in got.items():
                worst[k] = max(worst.get(k, 0.0), O.rowfrac(v[has], c['ref'][k][has]))
            worst['lse'] = max(worst.get('lse', 0.0), O.lsefrac(torch.logsumexp(s, -1).numpy()[has], c['ref']['lse'][has]))
    for D in (4, 3):                                                         # the large-score inputs of the GPU file
        x, q, dc = O.large_scores(D, trip + 3)
        ref = O.run(x, q, scale=1.0, dc=dc)
        xt, qt = (torch.tensor(v, requires_grad=True) for v in (x, q))
        out = _compose(xt, qt, torch.ones(x.shape[:2], dtype=torch.bool), 1.0)
        dx, dq = torch.autograd.grad(out, (xt, qt), torch.tensor(dc))
        for k, v in (('out', out.detach()), ('dx', dx), ('dq', dq)):
            worst['large ' + k] = max(worst.get('large ' + k, 0.0), O.rowfrac(v.numpy(), ref[k]))
    print('fp32 composition, worst fraction of the GPU bounds: %s' % ', '.join('%s %.3f' % kv for kv in sorted(worst.items())))
    assert all(v <= 0.5 for v in worst.values()), worst
