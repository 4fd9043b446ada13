"""GPU: CartesianProductLayer's CrossedIds through the crossed-id kernels (csrc/cross_hash.hip).  Texts and bucket numbers are compared with
the plain-Python oracle of tests/_cross_oracle.py; embeddings and gradients are compared BIT FOR BIT with the same layer called on the
host-composed strings: that route hashes on the host and enters the same gather code, so there is no tolerance.

Shapes are the smallest at which a path can go wrong: B 3 with dims (2, 3, 2); B 43 with dims (3, 2), 258 elements = one full tile of 256 plus
two; a first input that is one shared row; pooled with P = 17 x 16 = 272, more than one 256-id piece per row; D 4 (16-byte lanes) and D 3 (scalar
lanes); 1, 2 and 5 hash functions (5 crosses the four-rows-in-flight group).  FastMultiHashLayer's unsalted hash takes 32 bytes, so its cases
cross two int32 inputs."""
import numpy as np
import pytest
import torch

import _cross_oracle as C
from test_cartesian_product_cpu import CASES, SEPARATORS

pytestmark = pytest.mark.gpu
COMBINERS = ('sum', 'mean', 'concat', None)


def hash_layers():
    from rec_now_amd.layers import FastMultiHashLayer, MultiHashLayer
    return {'multi': MultiHashLayer, 'fast': FastMultiHashLayer}


def cross(arrays, dev, separator='-', patterns=None, default=''):
    from rec_now_amd.layers import CartesianProductLayer, CrossedIds
    out = CartesianProductLayer(separator=separator)([torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays], patterns, default)
    assert isinstance(out, CrossedIds)
    return out


def make_layer(kind, num_bins, D, num_hash, dev, rng, trainable=True):
    layer = hash_layers()[kind](num_bins, D, num_hash=num_hash, salts=3, trainable=trainable)
    layer._build_device = dev
    layer.build()
    with torch.no_grad():
        for t in layer.tables:
            t.copy_(torch.from_numpy((rng.standard_normal(tuple(t.shape)) * 0.5).astype(np.float32)))
    return layer


def pattern_on_small_input(arrays, pattern):
    """An invalid-pattern list with `pattern` on the first input of small ids (the random 19-digit ones never meet a literal)."""
    k = [i for i, a in enumerate(arrays) if np.abs(a).max() < 100][0]
    return [pattern if i == k else None for i in range(len(arrays))]


def same(a, b):
    return a.shape == b.shape and a.tolist() == b.tolist()


def bits(t):
    return t.detach().cpu().numpy()


# ---- texts ---------------------------------------------------------------------------------------------------------------------------------
def test_texts_equal_the_oracle(dev, golden):
    for sep in SEPARATORS:
        for name, arrays in CASES:
            cr = cross(arrays, dev, sep)
            want = C.texts(arrays, sep)
            assert cr.shape == want.shape
            assert same(cr.numpy(), want), (name, sep)
            text, lens = cr.text_bytes()
            assert text.dtype == torch.uint8 and lens.dtype == torch.int32 and text.is_cuda and lens.is_cuda
            W = max(8, -(-cr.worst_text_bytes // 8) * 8)
            assert tuple(text.shape) == want.shape + (W,) and tuple(lens.shape) == want.shape
            text, lens = bits(text), bits(lens)
            assert lens.reshape(-1).tolist() == [len(t) for t in want.reshape(-1)]
            assert all(not row[n:].any() for row, n in zip(text.reshape(-1, W), lens.reshape(-1))), 'not zero padded'
    g = golden('cartesian')
    digits = [g['digits_in1'], g['digits_in2'], g['digits_in3']]
    got = cross(digits, dev, '').numpy()
    assert np.array_equal(np.array([[float(v) for v in r] for r in got], dtype=np.float32), g['digits_out'])
    # replaced elements read as the default string, also one longer than every text
    ids = [np.array([[5, -1, 1]] * 2, dtype=np.int32), np.array([[-1, 1, 2], [11, -11, 0]], dtype=np.int32)]
    for pl, default in (([None, '1'], 'X'), (['1|-1', ''], 'a default string of more than twenty-six bytes'), (['', None], '')):
        assert same(cross(ids, dev, '-', pl, default).numpy(), C.texts(ids, '-', pl, default)), pl


# ---- bucket numbers -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['multi', 'fast'])
def test_bucket_numbers_equal_the_oracle(dev, kind):
    rng = np.random.default_rng(20)
    big = dict(multi=np.int64, fast=np.int32)[kind]
    info = np.iinfo(big)
    cases = [[rng.integers(info.min, info.max, (43, 3), dtype=big), rng.integers(-20, 20, (43, 2), dtype=np.int32)],
             [rng.integers(-20, 20, (1, 4), dtype=np.int32), rng.integers(info.min, info.max, (5, 3), dtype=big)]]
    if kind == 'multi':
        cases.append([rng.integers(info.min, info.max, (3, 2), dtype=big), rng.integers(-5, 5, (3, 3), dtype=np.int32), rng.integers(0, 99, (3, 2))])
    for arrays in cases:
        for pl, default in ((None, ''), (pattern_on_small_input(arrays, '1|-1|0'), 'na')):
            texts = C.texts(arrays, '-', pl, default)
            cr = cross(arrays, dev, '-', pl, default)
            for nh in (1, 2, 5):
                layer = hash_layers()[kind](1000, -1, num_hash=nh, salts=3)
                want = C.buckets(texts, 1000, nh, 3, kind == 'fast')                      # (B, P, nh)
                for combiner in COMBINERS:
                    got, ref = layer(cr, combiner=combiner), layer(texts, combiner=combiner)          # the string route hashes on the host
                    if isinstance(ref, list):
                        assert len(got) == len(ref) == nh and all(g.is_cuda and np.array_equal(bits(g), bits(r)) for g, r in zip(got, ref))
                        assert all(np.array_equal(bits(g), want[..., h]) for h, g in enumerate(got))
                    else:
                        assert got.is_cuda and got.dtype == torch.int64 and np.array_equal(bits(got), bits(ref)), (kind, nh, combiner)
                        assert np.array_equal(bits(got), np.concatenate([want[..., h] for h in range(nh)], axis=-1)), (kind, nh, combiner)


# ---- embeddings and gradients: bit for bit the string route -----------------------------------------------------------------------------------
def _embed_cases(kind, rng):
    """(tag, arrays, num_hash, D)"""
    big = dict(multi=np.int64, fast=np.int32)[kind]
    info = np.iinfo(big)
    wide = lambda shape: rng.integers(info.min, info.max, shape, dtype=big)           # noqa: E731

    def small(shape):
        """ids near zero; 1 and -1 (what the invalid patterns of the test name) and 5 (what they do not) are always among them"""
        a = rng.integers(-12, 12, shape, dtype=np.int32)
        a.flat[0], a.flat[a.size // 2], a.flat[-1] = 1, 5, -1
        return a

    cases = [('B43 (3, 2)', [wide((43, 3)), small((43, 2))], 2, 3),
             ('shared row (3, 4)', [small((1, 3)), wide((5, 4))], 1, 4),
             ('pooled pieces (17, 16)', [small((3, 17)), wide((3, 16))], 2, 4),
             ('B3 (6, 2)', [wide((3, 6)), small((3, 2))], 5, 4)]
    if kind == 'multi':
        cases.append(('B3 (2, 3, 2)', [wide((3, 2)), small((3, 3)), rng.integers(0, 1 << 40, (3, 2))], 5, 4))
    return cases


def _run(layer, ids, mode, w, dy_of):
    """forward + backward of one mode -> (outputs, d tables, d weights) as numpy."""
    for t in layer.tables:
        t.grad = None
    wt = None
    if mode == 'pooled':
        wt = w.clone().requires_grad_(True)
        out = layer.get_pooling(ids, wt)
    elif mode == 'get':
        out = layer.get(ids)
    else:
        out = layer(ids, combiner=mode)
    outs = out if isinstance(out, list) else [out]
    torch.autograd.backward(outs, [dy_of(o) for o in outs])
    return [bits(o) for o in outs], [bits(t.grad) for t in layer.tables], (bits(wt.grad) if wt is not None else None)


@pytest.mark.parametrize('patterns', [False, True])
@pytest.mark.parametrize('kind', ['multi', 'fast'])
def test_embeddings_and_gradients_equal_the_string_route(dev, kind, patterns):
    rng = np.random.default_rng(22)
    for tag, arrays, nh, D in _embed_cases(kind, rng):
        # negative ids under '-': "5--1" and the like reach the matcher
        pl, default = (pattern_on_small_input(arrays, '1|-1|11'), 'na') if patterns else (None, '')
        texts = C.texts(arrays, '-', pl, default)
        if patterns:
            plain = C.texts(arrays, '-')
            n_hit = sum(a != b for a, b in zip(texts.reshape(-1), plain.reshape(-1)))
            assert 0 < n_hit < texts.size, tag
        cr = cross(arrays, dev, '-', pl, default)
        layer = make_layer(kind, 37, D, nh, dev, rng)
        B, P = texts.shape
        w = torch.from_numpy(rng.standard_normal((B, P)).astype(np.float32)).to(dev)
        gen = torch.Generator().manual_seed(5)
        for mode in COMBINERS + ('get', 'pooled'):
            grads = {}
            dy_of = lambda o: grads.setdefault(tuple(o.shape), torch.randn(tuple(o.shape), generator=gen).to(dev))       # noqa: E731
            got = _run(layer, cr, mode, w, dy_of)
            ref = _run(layer, texts, mode, w, dy_of)
            what = '%s %s nh%d D%d %s' % (kind, tag, nh, D, mode)
            assert len(got[0]) == len(ref[0]) and all(np.array_equal(a, b) for a, b in zip(got[0], ref[0])), what + ' forward'
            assert all(np.array_equal(a, b) for a, b in zip(got[1], ref[1])), what + ' d table'
            assert any(a.any() for a in got[1]), what + ' d table is zero'
            if mode == 'pooled':
                assert got[0][0].shape == (B, D) and np.array_equal(got[2], ref[2]) and got[2].any(), what + ' d weights'
            elif mode in ('sum', 'mean', 'get'):
                assert got[0][0].shape == (B, P, D), what


@pytest.mark.parametrize('kind', ['multi', 'fast'])
def test_table_gradient_is_bit_identical_over_two_runs(dev, kind):
    rng = np.random.default_rng(24)
    layer = make_layer(kind, 3, 8, 2, dev, rng)                                       # 3 bins: every row collects hundreds of entries
    cr = cross([rng.integers(0, 1 << 20, (64, 10), dtype=np.int32), rng.integers(0, 1 << 20, (64, 5), dtype=np.int32)], dev)
    w = torch.randn(64, 50, device=dev, requires_grad=True)
    dy = torch.randn(64, 8, device=dev)
    runs = []
    for _ in range(2):
        for x in layer.tables:
            x.grad = None
        w.grad = None
        out = layer.get_pooling(cr, w)
        out.backward(dy)
        runs.append([bits(out), bits(w.grad)] + [bits(x.grad) for x in layer.tables])
    assert all(np.array_equal(a, b) for a, b in zip(*runs))


def test_frozen_table_takes_no_keys(dev):
    from rec_now_amd.layers import multi_hash_layer as M
    rng = np.random.default_rng(26)
    cr = cross([rng.integers(0, 1 << 40, (64, 5)), rng.integers(0, 9, (64, 2))], dev)
    calls = []
    real = M._lib.call
    M._lib.call = lambda name, *a: (calls.append((name, a)), real(name, *a))[1]
    try:
        frozen = make_layer('multi', 100, 8, 2, dev, rng, trainable=False)
        out = frozen.get_pooling(cr, torch.ones(64, 10, device=dev))
        assert not out.requires_grad
        fwd = [a for n, a in calls if n == 'recnow_cross_hash_embed_fwd']
        assert len(fwd) == 1 and fwd[0][11] is None and fwd[0][12] is None            # no keys written
        assert not any(n == 'recnow_hash_embed_fwd' for n, _ in calls)
        del calls[:]
        w = torch.ones(64, 10, device=dev, requires_grad=True)
        frozen.get_pooling(cr, w).sum().backward()
        names = [n for n, _ in calls]
        assert 'recnow_hash_embed_bwd_weights' in names and 'recnow_embed_rows_bwd_direct' not in names and w.grad is not None
        fwd = [a for n, a in calls if n == 'recnow_cross_hash_embed_fwd']
        assert fwd[0][11] is not None and fwd[0][12] is None                          # d weights re-gathers from the 64-bit keys only
    finally:
        M._lib.call = real


@pytest.mark.parametrize('kind', ['multi', 'fast'])
def test_empty_batch(dev, kind):
    rng = np.random.default_rng(28)
    layer = make_layer(kind, 10, 4, 2, dev, rng)
    cr = cross([np.zeros((0, 3), dtype=np.int32), np.zeros((0, 2), dtype=np.int32)], dev)
    assert cr.shape == (0, 6) and cr.numpy().shape == (0, 6)
    text, lens = cr.text_bytes()
    assert tuple(text.shape) == (0, 6, 24) and tuple(lens.shape) == (0, 6)
    assert tuple(layer(cr).shape) == (0, 6, 4)
    assert tuple(layer.get_pooling(cr, torch.zeros((0, 6), device=dev)).shape) == (0, 4)
    layer(cr).sum().backward()
    assert all(x.grad is not None and float(x.grad.abs().sum()) == 0.0 for x in layer.tables)
    assert tuple(hash_layers()[kind](10, -1)(cr, combiner='concat').shape) == (0, 12)
