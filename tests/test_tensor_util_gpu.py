"""GPU: PoolingLayer, pad_or_truncate / FixLengthLayer and the element-wise embedding weights (csrc/tensor_util.hip) against the numpy fp64 oracle
of tests/_tensor_util_oracle.py and the reference's own unit-test literals (tests/golden/tensor_util.npz).

Copies (pad / truncate and its gradient, the gathered weights) and max / min must be bit-identical; sums (sum / mean, apply, every other gradient)
stay within 1e-5 of the oracle tensor's largest magnitude, the project's standing parity bound (PARITY of tests/test_slot_util_gpu.py).  Sum / mean
inputs are drawn from N(0.5, 1), so the scale of a result grows with the reduced length and the bound is no bound on cancellation noise; max / min
inputs are whole numbers in -2 .. 2, so ties occur in most runs."""
import itertools

import numpy as np
import pytest
import torch

import _tensor_util_oracle as O

pytestmark = pytest.mark.gpu

PARITY = 1e-5
COMBINERS = ['sum', 'mean', 'max', 'min']


def _close(got, want, what):
    got, want = got.detach().cpu().double().numpy(), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, '%s: shape %s, expected %s' % (what, got.shape, want.shape)
    err, scale = (np.abs(got - want).max() if got.size else 0.0), max(np.abs(want).max() if want.size else 0.0, 1e-30)
    print('%s: max err %.3g, scale %.3g' % (what, err, scale))
    assert err <= PARITY * scale, '%s: max err %.3g vs scale %.3g' % (what, err, scale)


def _same(got, want, what):
    got, want = got.detach().cpu().numpy(), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, '%s: %s %s, expected %s %s' % (what, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want), what


def _draw(rng, shape, combiner):
    if combiner in ('sum', 'mean'):
        return rng.normal(0.5, 1.0, shape).astype(np.float32)
    return rng.integers(-2, 3, shape).astype(np.float32)


def _grad(rng, shape):
    return np.asarray(rng.normal(size=shape), dtype=np.float32)


def _pool(dev, x, axis, keepdims, combiner, g=None):
    """(output, d input) of the layer on the numpy input x; g: the output gradient (numpy) or None for a forward alone."""
    from rec_now_amd.layers import PoolingLayer
    t = (x if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(dev)).requires_grad_(g is not None)
    y = PoolingLayer(axis=axis, keepdims=keepdims, combiner=combiner)(t)
    if g is None:
        return y, None
    y.backward(torch.from_numpy(g).to(dev))
    return y, t.grad


# ---- the reference's own cases -----------------------------------------------------------------------------------------------------------------
def test_reference_fixture_cases(dev, golden):
    from rec_now_amd.layers import FixLengthLayer, PoolingLayer
    from rec_now_amd.rec_block.embedding_wise_weight import gather_embedding_element_wise_weight
    g = golden('tensor_util')
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                   # noqa: E731
    x = put(g['pool_in'])
    _same(PoolingLayer(axis=0, keepdims=True, combiner='sum')(x), g['pool_axis0_keepdims_sum'], 'PoolingLayer axis 0')
    _same(PoolingLayer(axis=1, keepdims=False, combiner='sum')(x), g['pool_axis1_sum'], 'PoolingLayer axis 1')
    layer = FixLengthLayer(length=int(g['fix_length']), axis=int(g['fix_axis']), name='FixLengthLayer')
    for case in ('truncate', 'pad', 'same'):
        _same(layer(put(g['fix_%s_in' % case])), g['fix_%s_out' % case], 'FixLengthLayer ' + case)
    _same(gather_embedding_element_wise_weight(put(g['elw_weights']), g['elw_pos_idx'].tolist()), g['elw_out'], 'element-wise weights')


# ---- PoolingLayer ------------------------------------------------------------------------------------------------------------------------------
def _factor(n):
    for a in (8, 9, 4, 2, 17):
        if n % a == 0 and n > a:
            return a, n // a
    return None


def _variants(O_, R, I):
    """(shape, axis) pairs of rank 2, 3 and 4 that all fold to (O_, R, I); negative and sequence axes among them."""
    out = [((O_, R, I), 1), ((O_, R, I), -2)]
    if I == 1:
        out.append(((O_, R), -1))
    if O_ == 1:
        out.append(((R, I), 0))
    if _factor(I):
        out.append(((O_, R) + _factor(I), -3))
    if _factor(R):
        out.append(((O_,) + _factor(R) + (I,), (1, 2)))
    if _factor(O_):
        out.append((_factor(O_) + (R, I), 2))
    return out


POOL_EXTENTS = list(itertools.product([1, 2, 37], [1, 2, 63, 64, 65, 257], [1, 3, 4, 5, 64, 68]))


@pytest.mark.parametrize('combiner', COMBINERS)
def test_pooling_equals_oracle(dev, combiner):
    rng = np.random.default_rng(COMBINERS.index(combiner))
    ranks = set()
    for k, (O_, R, I) in enumerate(POOL_EXTENTS):
        variants = _variants(O_, R, I)
        for keepdims in (False, True):
            shape, axis = variants[(k + keepdims) % len(variants)]
            ranks.add(len(shape))
            x = _draw(rng, shape, combiner)
            want = O.reduce_axis(x, axis, keepdims, combiner)
            g = _grad(rng, want.shape)
            y, dx = _pool(dev, x, axis, keepdims, combiner, g)
            what = '%s of %s over %s keepdims=%s' % (combiner, shape, axis, keepdims)
            assert y.dtype == torch.float32 and tuple(y.shape) == want.shape, what
            if combiner in ('max', 'min'):
                _same(y, want.astype(np.float32), what)
            else:
                _close(y, want, what)
            _close(dx, O.reduce_axis_grad(x, axis, keepdims, combiner, g), 'd ' + what)
    assert ranks == {2, 3, 4}


@pytest.mark.parametrize('combiner', ['max', 'min'])
def test_tie_gradient_is_shared_equally_position_by_position(dev, combiner):
    rng = np.random.default_rng(7)
    for O_, R, I in ((37, 65, 1), (2, 257, 4), (37, 64, 5), (1, 70000, 1), (300, 5, 3), (2, 300, 68)):
        x = _draw(rng, (O_, R, I), combiner)
        g = rng.normal(size=(O_, I)).astype(np.float32)
        _, dx = _pool(dev, x, 1, False, combiner, g)
        dx = dx.cpu().numpy()
        best = x.max(1) if combiner == 'max' else x.min(1)
        ties = 0
        for o, i in itertools.product(range(O_), range(I)):
            hit = x[o, :, i] == best[o, i]
            count = int(hit.sum())
            ties += count > 1
            share = np.float64(g[o, i]) / count
            assert np.all(dx[o, ~hit, i] == 0.0), (O_, R, I, o, i)
            assert np.all(np.abs(dx[o, hit, i] - share) <= PARITY * abs(share)), (O_, R, I, o, i, count)
        assert ties > 0


@pytest.mark.parametrize('n', [1, 255, 256, 257, 65537, 1000003])
def test_pooling_of_all_elements_and_of_one_row(dev, n):
    rng = np.random.default_rng(n)
    for combiner in COMBINERS:
        x = _draw(rng, (n,), combiner)
        for shape, axis, keepdims in (((n,), None, False), ((1, n), 1, True), ((n,), None, True)):
            if n > 65537 and keepdims and axis is None:
                continue
            xs = x.reshape(shape)
            want = O.reduce_axis(xs, axis, keepdims, combiner)
            g = _grad(rng, want.shape)
            y, dx = _pool(dev, xs, axis, keepdims, combiner, g)
            what = '%s of %s over %s keepdims=%s' % (combiner, shape, axis, keepdims)
            assert tuple(y.shape) == want.shape, what
            if combiner in ('max', 'min'):
                _same(y, want.astype(np.float32), what)
            else:
                _close(y, want, what)
            _close(dx, O.reduce_axis_grad(xs, axis, keepdims, combiner, g), 'd ' + what)
    if n == 257:                                   # axis=None of a matrix: all elements, scalar result
        x = _draw(rng, (n, 5), 'sum')
        y, dx = _pool(dev, x, None, False, 'sum', np.full((), 2.0, dtype=np.float32))
        assert tuple(y.shape) == ()
        _close(y, O.reduce_axis(x, None, False, 'sum'), 'sum of all elements of a matrix')
        _close(dx, np.full(x.shape, 2.0), 'd sum of all elements')


def test_pooling_is_bit_identical_from_run_to_run(dev):
    rng = np.random.default_rng(3)
    for combiner in COMBINERS:
        for shape, axis in (((37, 257, 68), 1), ((2, 4001, 4), 1), ((300, 65), 1), ((1000003,), None), ((5, 3000, 3), 1)):
            x = torch.from_numpy(_draw(rng, shape, combiner)).to(dev)
            want = O.reduce_axis(x.cpu().numpy(), axis, False, combiner)
            g = _grad(rng, want.shape)
            runs = [_pool(dev, x.clone(), axis, False, combiner, g) for _ in range(2)]
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), (combiner, shape)
            _close(runs[0][0], want, '%s of %s' % (combiner, shape))


def test_pooling_takes_non_contiguous_and_empty_inputs(dev):
    rng = np.random.default_rng(4)
    x = _draw(rng, (65, 37, 4), 'sum')
    t = torch.from_numpy(x).to(dev).permute(1, 0, 2)
    assert not t.is_contiguous()
    y, _ = _pool(dev, t, 1, False, 'sum')
    _close(y, O.reduce_axis(x.transpose(1, 0, 2), 1, False, 'sum'), 'sum of a permuted tensor')
    for shape, axis in (((0, 5, 3), 1), ((4, 5, 0), 1), ((0, 5), -1)):
        y, dx = _pool(dev, np.zeros(shape, dtype=np.float32), axis, True, 'max', np.zeros(O.reduce_axis(np.zeros(shape), axis, True, 'sum').shape, dtype=np.float32))
        assert y.numel() == 0 and tuple(dx.shape) == shape
    with pytest.raises(ValueError, match='empty axis'):
        _pool(dev, np.zeros((4, 0, 3), dtype=np.float32), 1, False, 'sum')


# ---- pad_or_truncate ---------------------------------------------------------------------------------------------------------------------------
PAD_EXTENTS = list(itertools.product([1, 37], [0, 1, 3, 64, 65], [1, 2, 64, 67], [1, 3, 4, 5, 32]))
PAD_DTYPES = [(np.float32, 2.5), (np.int32, -7), (np.int64, (1 << 40) + 3)]


def _pad_layout(O_, L, I, k):
    """(shape, axis) with the padded axis first (O_ == 1), last (I == 1) or in the middle; a rank-4 layout for I == 32."""
    if O_ == 1 and k % 2 == 0:
        return ((L, I), 0) if I > 1 else ((L,), 0)
    if I == 1 and k % 2 == 0:
        return (O_, L), -1
    if I == 32:
        return (O_, L, 4, 8), (1 if k % 4 < 2 else -3)
    return (O_, L, I), 1


@pytest.mark.parametrize('dtype,fill', PAD_DTYPES)
def test_pad_or_truncate_equals_oracle(dev, dtype, fill):
    from rec_now_amd.layers import FixLengthLayer
    from rec_now_amd.layers.fix_length_layer import pad_or_truncate
    rng = np.random.default_rng(11)
    seen = set()
    for k, (O_, L_in, L_out, I) in enumerate(PAD_EXTENTS):
        shape, axis = _pad_layout(O_, L_in, I, k)
        seen.add((len(shape), 'first' if axis % len(shape) == 0 else 'last' if axis % len(shape) == len(shape) - 1 else 'middle'))
        x = (rng.normal(size=shape) * 100).astype(dtype)
        t = torch.from_numpy(x).to(dev)
        what = '%s %s axis %d: %d -> %d' % (np.dtype(dtype).name, shape, axis, L_in, L_out)
        if dtype == np.float32:
            t.requires_grad_(True)
        y = pad_or_truncate(t, L_out, axis, fill) if k % 2 else FixLengthLayer(L_out, axis, constant_values=fill)(t)
        if L_out == L_in:
            assert y is t, what
            continue
        want = O.pad_or_truncate(x, L_out, axis, fill)
        _same(y, want, what)
        if L_in == 0:
            assert want.size == 0 or bool(np.all(want == np.asarray(fill, dtype=dtype))), what
        if dtype == np.float32:
            g = _grad(rng, want.shape)
            y.backward(torch.from_numpy(g).to(dev))
            _same(t.grad, O.pad_or_truncate_grad(shape, L_out, axis, g), 'd ' + what)
        else:
            assert not y.requires_grad
    assert {s[1] for s in seen} == {'first', 'middle', 'last'}


def test_pad_or_truncate_of_a_non_contiguous_input_and_default_arguments(dev):
    from rec_now_amd.layers.fix_length_layer import pad_or_truncate
    rng = np.random.default_rng(12)
    x = rng.normal(size=(65, 37, 4)).astype(np.float32)
    t = torch.from_numpy(x).to(dev).permute(1, 2, 0)                                     # (37, 4, 65), strides out of order
    assert not t.is_contiguous()
    xt = x.transpose(1, 2, 0)
    _same(pad_or_truncate(t, 67), O.pad_or_truncate(xt, 67, -1, 0), 'permuted input, default axis and constant')
    _same(pad_or_truncate(t, 3, axis=1), O.pad_or_truncate(xt, 3, 1, 0), 'permuted input, truncated')
    ids = torch.from_numpy(rng.integers(-5, 5, (37, 80))).to(dev)[:, ::2]                # a strided int64 view
    _same(pad_or_truncate(ids, 50, constant_values=-1), O.pad_or_truncate(ids.cpu().numpy(), 50, -1, -1), 'strided int64 view')
    same = torch.zeros(5, 3, device=dev)
    assert pad_or_truncate(same, 3) is same and pad_or_truncate(same, 5, axis=0) is same
    for shape, length, axis in (((0, 3), 4, 1), ((4, 3, 0), 5, 1), ((4, 3), 0, 1)):     # empty outer / inner extent, length 0
        y = pad_or_truncate(torch.zeros(shape, device=dev), length, axis, 1.0)
        assert tuple(y.shape) == O.pad_or_truncate(np.zeros(shape), length, axis).shape


# ---- element-wise weights ----------------------------------------------------------------------------------------------------------------------
def _tables(rng, E):
    """Position tables over E embeddings: widths 1 .. 17 per embedding in order; one with an embedding absent and a length that is a multiple of 4;
    one unsorted."""
    widths = rng.integers(1, 18, E)
    ordered = np.repeat(np.arange(E), widths)
    absent = ordered[ordered != E // 2] if E > 1 else ordered
    absent = np.concatenate([absent, np.full(-len(absent) % 4, E - 1)])
    mixed = rng.permutation(ordered)
    if np.array_equal(mixed, ordered):
        mixed = ordered[::-1]
    return [ordered.tolist(), absent.tolist(), mixed.tolist()]


ELW_SHAPES = list(itertools.product([1, 37, 300], [1, 3, 64, 65, 200])) + [(5, 5000)]   # E = 5000: rows too wide for the LDS stage


@pytest.mark.parametrize('B,E', ELW_SHAPES)
def test_element_wise_weights_equal_oracle(dev, B, E):
    from rec_now_amd.rec_block.embedding_wise_weight import apply_embedding_element_wise_weight, gather_embedding_element_wise_weight
    rng = np.random.default_rng(B * 1000 + E)
    tables = _tables(rng, E) if E <= 200 else [rng.integers(0, E, 300).tolist(), rng.integers(0, E, 301).tolist()]
    if E > 1 and E <= 200:
        assert E // 2 not in tables[1] and len(tables[1]) % 4 == 0 and tables[2] != sorted(tables[2])
    for n, pos in enumerate(tables):
        P = len(pos)
        w = rng.normal(size=(B, E)).astype(np.float32)
        x = rng.normal(size=(B, P)).astype(np.float32)
        g = rng.normal(size=(B, P)).astype(np.float32)
        tg = torch.from_numpy(g).to(dev)
        what = 'B=%d E=%d P=%d table %d' % (B, E, P, n)
        table = [pos, tuple(pos), np.array(pos), torch.tensor([pos])][(n + B) % 4]
        runs = []
        for _ in range(2):
            tw = torch.from_numpy(w).to(dev).requires_grad_(True)
            tx = torch.from_numpy(x).to(dev).requires_grad_(True)
            gathered = gather_embedding_element_wise_weight(tw, table)
            _same(gathered, O.gather_weight(w, pos), 'gather ' + what)
            gathered.backward(tg)
            dw_gather = tw.grad.clone()
            tw.grad = None
            applied = apply_embedding_element_wise_weight(tx, tw, table)
            assert torch.equal(applied, tx.detach() * gathered.detach()), 'apply == inputs * gather, ' + what
            applied.backward(tg)
            runs.append((dw_gather, tw.grad.clone(), tx.grad.clone()))
        for a, b in zip(*runs):
            assert torch.equal(a, b), 'backward run to run, ' + what
        _close(applied, O.apply_weight(x, w, pos), 'apply ' + what)
        _close(runs[0][0], O.elem_weight_grads(None, w, pos, g)[0], 'd gather / d weights ' + what)
        dw, dx = O.elem_weight_grads(x, w, pos, g)
        _close(runs[0][1], dw, 'd apply / d weights ' + what)
        _close(runs[0][2], dx, 'd apply / d inputs ' + what)


def test_element_wise_weights_partial_gradients_and_empty_extents(dev):
    from rec_now_amd.rec_block.embedding_wise_weight import apply_embedding_element_wise_weight, gather_embedding_element_wise_weight
    rng = np.random.default_rng(13)
    B, E, pos = 37, 5, [4, 0, 0, 2, 2, 2, 4]
    w, x, g = (rng.normal(size=s).astype(np.float32) for s in ((B, E), (B, 7), (B, 7)))
    dw, dx = O.elem_weight_grads(x, w, pos, g)
    tw, tx = torch.from_numpy(w).to(dev), torch.from_numpy(x).to(dev).requires_grad_(True)
    apply_embedding_element_wise_weight(tx, tw, pos).backward(torch.from_numpy(g).to(dev))            # only the inputs want a gradient
    _close(tx.grad, dx, 'd inputs alone')
    tw, tx = torch.from_numpy(w).to(dev).requires_grad_(True), torch.from_numpy(x).to(dev)
    apply_embedding_element_wise_weight(tx, tw, pos).backward(torch.from_numpy(g).to(dev))            # only the weights
    _close(tw.grad, dw, 'd weights alone')
    assert float(tw.grad[:, 1].abs().sum()) == 0.0 and float(tw.grad[:, 3].abs().sum()) == 0.0       # absent embeddings: exact zeros
    assert tuple(gather_embedding_element_wise_weight(torch.zeros(0, 3, device=dev), [0, 2]).shape) == (0, 2)
    tw = torch.from_numpy(w).to(dev).requires_grad_(True)
    out = gather_embedding_element_wise_weight(tw, [])
    assert tuple(out.shape) == (B, 0)
    out.sum().backward()
    assert tuple(tw.grad.shape) == (B, E) and float(tw.grad.abs().sum()) == 0.0
    with pytest.raises(ValueError):
        gather_embedding_element_wise_weight(tw, torch.tensor([0, 5], device=dev))


# ---- composition and graph capture -------------------------------------------------------------------------------------------------------------
def test_pad_pool_apply_chain_is_graph_capturable(dev):
    """No hidden sync, no host-side size: pad_or_truncate -> PoolingLayer('mean', axis=1) -> apply_embedding_element_wise_weight is captured once
    (single stream) and replayed twice on new input contents; each replay equals the eager result bit for bit."""
    from rec_now_amd.layers import PoolingLayer
    from rec_now_amd.layers.fix_length_layer import pad_or_truncate
    from rec_now_amd.rec_block.embedding_wise_weight import apply_embedding_element_wise_weight
    rng = np.random.default_rng(61)
    B, L, D, E = 300, 37, 32, 5
    pos = np.repeat(np.arange(E), [3, 9, 1, 12, 7]).tolist()
    assert len(pos) == D
    draw = lambda: (rng.normal(0.5, 1.0, (B, L, D)).astype(np.float32), rng.normal(size=(B, E)).astype(np.float32))      # noqa: E731
    tx, tw = (torch.from_numpy(a).to(dev) for a in draw())
    pool = PoolingLayer(axis=1, combiner='mean')

    def step():
        with torch.no_grad():
            return apply_embedding_element_wise_weight(pool(pad_or_truncate(tx, 50, axis=1)), tw, pos)
    step()                                              # the (cached) upload of the position table happens outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for _ in range(2):
        x, w = draw()                                   # new contents, same storage
        tx.copy_(torch.from_numpy(x).to(dev))
        tw.copy_(torch.from_numpy(w).to(dev))
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        want = step()
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        _close(got, O.apply_weight(O.reduce_axis(O.pad_or_truncate(x, 50, 1, 0), 1, False, 'mean'), w, pos), 'replayed chain')
