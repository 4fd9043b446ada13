"""GPU: attention_by_softmax (csrc/attention_softmax.hip) and TargetAttentionLayer against the fp64 oracle of tests/_attention_softmax_oracle.py,
on both routes, every instantiation and both directions.

Bounds: per row 1e-5 max(1, largest |reference| entry of that row) for out, dx (a row is a position), dquery and the layer's output and input
gradients; the layer's weight gradients per tensor; lse within 1e-6 max(1, |lse|).  No entry is left out of a comparison.  The plain fp32 torch
composition on the CPU stays under 0.06 of the row bounds and 0.2 of the lse bound on every shape and mode of this file
(tests/test_attention_softmax_cpu.py holds it under half).  Shapes are placed from recnow_attention_softmax_tile (_attention_softmax_oracle.shapes):
a wave that is full, ragged or holds one sample; a position loop of exactly one trip, one trip plus one piece, several; every D class of both
routes.  Each shape runs with no mask, lengths, a mask, and both; sample 0 is always full-length and, in every mode that can mask, the last sample
is empty (B = 1: the one sample is full; empty samples alone are in test_an_empty_sample_in_every_slot).
Every comparison prints its fraction of the bound; the largest per tensor are printed once more by the last test of the file."""
import math

import numpy as np
import pytest
import torch

import _attention_softmax_oracle as O

pytestmark = pytest.mark.gpu
WORST = {}


def _lib():
    from rec_now_amd import _lib as L
    return L


def _tile():
    lib = _lib().load()
    return tuple(lib.recnow_attention_softmax_tile(i) for i in range(3))


SPW, TRIP, LANES = _tile()
SHAPES = O.shapes(SPW, TRIP, LANES)


def _op(*a, **k):
    from rec_now_amd.rec_block.attention import attention_by_softmax
    return attention_by_softmax(*a, **k)


def _gpu(a, dev, grad=False):
    if a is None:
        return None
    t = torch.from_numpy(np.array(a)).to(dev)                               # a copy: the shared cases are read-only
    return t.requires_grad_(True) if grad else t


def _np(t):
    return t.detach().cpu().numpy()


def _hold(what, got, ref, group, frac=O.rowfrac):
    f = frac(_np(got) if isinstance(got, torch.Tensor) else got, ref)
    print('%-44s %.3f of the bound' % (what, f))
    WORST[group] = max(WORST.get(group, 0.0), f)
    assert f <= 1.0, '%s: %.3f of the bound' % (what, f)


def _route(which, B, L, D, H, *tensors):
    """The route of a call, from the alignment of the tensors it is given (user, query, out[, dout, duser, dquery])."""
    mis = sum(1 << i for i, t in enumerate(tensors) if t is not None and t.data_ptr() % 16 != 0)
    return _lib().load().recnow_attention_softmax_route(which, B, L, D, H, mis)


def _expected_route(D, H, vec_ok=True):
    hb = 1 if H <= 1 else 2 if H <= 2 else 4 if H <= 4 else 8
    if vec_ok and D % 4 == 0 and D // 4 in (1, 2, 4, 8, 16):
        return 200000 + 100 * (D // 4) + hb
    return 100000 + 100 * (16 if D <= 16 else 32 if D <= 32 else 64) + hb


def _run(dev, x, q, dc, lengths=None, mask=None, scale=None, grad_x=True, grad_q=True):
    """-> dict(out, lse, dx, dq) of numpy arrays (dx / dq None when not asked for) and the tensors of the call."""
    xt, qt, dct = _gpu(x, dev, grad_x), _gpu(q, dev, grad_q), _gpu(dc, dev)
    out, lse = _op(xt, qt, lengths=_gpu(lengths, dev), mask=_gpu(mask, dev), scale=scale, return_lse=True)
    assert not lse.requires_grad
    leaves = [t for t, on in ((xt, grad_x), (qt, grad_q)) if on]
    grads = list(torch.autograd.grad(out, leaves, dct)) if leaves else []
    dx = grads.pop(0) if grad_x else None
    dq = grads.pop(0) if grad_q else None
    torch.cuda.synchronize()
    return dict(out=_np(out), lse=_np(lse), dx=None if dx is None else _np(dx), dq=None if dq is None else _np(dq),
                tensors=(xt, qt, out, dct, dx, dq))


def _check(tag, got, ref, group):
    _hold(tag + ' out', got['out'], ref['out'], group + ' out')
    _hold(tag + ' lse', got['lse'], ref['lse'], group + ' lse', O.lsefrac)
    if got['dx'] is not None:
        _hold(tag + ' dx', got['dx'], ref['dx'], group + ' dx')
        assert not got['dx'][~ref['key']].any(), 'a dx row outside the keys is not zero'
    if got['dq'] is not None:
        _hold(tag + ' dq', got['dq'], ref['dq'], group + ' dq')
    empty = ~ref['key'].any(1)
    assert not got['out'][empty].any() and np.isneginf(got['lse'][empty]).all()
    assert got['dq'] is None or not got['dq'][empty].any()


# ---- every shape, every mode ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', O.MODES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'B%d-L%d-D%d-H%d' % s)
def test_matches_the_oracle(dev, shape, mode):
    B, L, D, H = shape
    c = O.case(B, L, D, H, mode)
    got = _run(dev, c['x'], c['q'], c['dc'], c['lengths'], c['mask'])
    xt, qt, out, dct, dx, dq = got['tensors']
    assert _route(0, B, L, D, H, xt, qt, out) == _expected_route(D, H) == _route(1, B, L, D, H, xt, qt, out, dct, dx, dq)
    kind = 'vector' if D % 4 == 0 and D // 4 in (1, 2, 4, 8, 16) else 'guarded'
    _check('%s %s' % (shape, mode), got, c['ref'], kind)
    assert got['out'].shape == (B, H, D) and got['lse'].shape == (B, H)


@pytest.mark.parametrize('H', [1, 2, 3, 8])
@pytest.mark.parametrize('D', [4, 8, 16, 32, 64, 3, 20, 65])
def test_every_instantiation_of_both_routes(dev, D, H):
    """The eight kernels per direction (five piece widths of the vector route, three lane groups of the guarded one) times the four head
    blocks: each is the route of this call, in both directions, and stays within the bounds."""
    B, L = SPW + 1, 9
    c = O.case(B, L, D, H, 'both', seed=3)
    got = _run(dev, c['x'], c['q'], c['dc'], c['lengths'], c['mask'])
    xt, qt, out, dct, dx, dq = got['tensors']
    want = _expected_route(D, H)
    assert _route(0, B, L, D, H, xt, qt, out) == want and _route(1, B, L, D, H, xt, qt, out, dct, dx, dq) == want
    _check('D %d H %d' % (D, H), got, c['ref'], 'instantiation')


def test_a_two_d_query_is_one_head_and_lengths_take_every_integer_form(dev):
    B, L, D = 5, 17, 8
    c = O.case(B, L, D, 1, 'lengths', seed=4)
    xt, qt = _gpu(c['x'], dev), _gpu(c['q'], dev)
    n = c['lengths']
    base, lse = _op(xt, qt, lengths=_gpu(n, dev), return_lse=True)
    for lengths in (n.astype(np.int32), n.reshape(B, 1), np.where(n == L, 2 ** 40, np.where(n == 0, -7, n))):
        out, l2 = _op(xt, qt[:, 0], lengths=_gpu(lengths, dev), return_lse=True)
        assert out.shape == (B, D) and l2.shape == (B,) and torch.equal(out, base[:, 0]) and torch.equal(l2, lse[:, 0])
    keys = np.arange(L)[None, :] < n[:, None]
    for m in (keys, keys.astype(np.float32) * -2.5, keys.astype(np.int64), keys.astype(np.uint8)):
        assert torch.equal(_op(xt, qt, mask=_gpu(m, dev)), base)
    quarter = _op(xt, qt, lengths=_gpu(n, dev), scale=0.25)
    assert torch.equal(_op(xt, qt * 0.5, lengths=_gpu(n, dev), scale=0.5), quarter)                # a power of two moves between q and scale


# ---- the exact regime ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('D', [4, 16, 5, 70])
def test_exact_regime_bit_for_bit(dev, D):
    """All keys of a sample are one integer vector, n = 1, 2, 4, 8 of them spread over two loop trips, scale 1/4, integer dc.  Every score of a
    sample is the same number, so every exponential is exp(0) = 1, the sum is n (its log2 an integer) and every product below is a small integer
    times a power of two -- exact in fp32 in any order: out is the key, dx = (sum_h dc_h) / n on the keys and 0 elsewhere, dquery = 0, bit for
    bit.  (Entries within +-4, D <= 70: every dot product is an integer below 2^11.)"""
    rng = np.random.default_rng(21)
    ns, L, H = (1, 2, 4, 8, 0), 70, 2
    B = len(ns)
    x = rng.integers(-4, 5, (B, L, D)).astype(np.float32)
    q = rng.integers(-4, 5, (B, H, D)).astype(np.float32)
    dc = rng.integers(-4, 5, (B, H, D)).astype(np.float32)
    key = np.zeros((B, L), dtype=np.uint8)
    want_out, want_dx = np.zeros((B, H, D), dtype=np.float32), np.zeros((B, L, D), dtype=np.float32)
    for b, n in enumerate(ns):
        rest = [int(l) for l in rng.permutation(L) if l not in (3, L - 1)]
        pos = np.array(([3, L - 1] + rest)[:n] if n >= 2 else rest[:n], dtype=np.int64)   # the first and the last (ragged) trip both hold keys
        key[b, pos] = 1
        x[b, pos] = x[b, pos[0]] if n else 0
        if n:
            want_out[b] = x[b, pos[0]]
            want_dx[b, pos] = dc[b].sum(0) / n
    got = _run(dev, x, q, dc, mask=key, scale=0.25)
    assert np.array_equal(got['out'], want_out), 'out is not the key bit for bit'
    assert np.array_equal(got['dx'], want_dx), 'dx is not dc / n bit for bit'
    assert np.array_equal(got['dq'], np.zeros_like(q)), 'dquery is not exactly zero'
    ref = O.run(x, q, mask=key, scale=0.25)
    _hold('exact regime D %d lse' % D, got['lse'], ref['lse'], 'exact lse', O.lsefrac)


# ---- large scores ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('D', [4, 3], ids=['vector', 'guarded'])
def test_large_scores_with_the_maximum_at_every_position(dev, D):
    """Scores of magnitude 100 from exactly representable inputs (_attention_softmax_oracle.large_scores, which also says how the backward is
    kept well conditioned): sample b has its largest score, 100, at position b, for every position of the first loop trip in turn and of the
    ragged last one (D = 4: one piece per position); head 1 negates the query.  An fp32 score carries no error here, so the 1e-5 bounds hold;
    the fp32 composition on the CPU sits at 0.05 of them (tests/test_attention_softmax_cpu.py)."""
    x, q, dc = O.large_scores(D, TRIP + 3)
    ref = O.run(x, q, scale=1.0, dc=dc)
    assert np.abs(ref['lse']).min() >= 100.0 and (ref['a'].argmax(-1)[:, 0] == np.arange(TRIP + 3)).all()
    _check('large scores D %d' % D, _run(dev, x, q, dc, scale=1.0), ref, 'large')


# ---- garbage outside the keys, NaN inside ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [(SPW + 1, TRIP // 2 + 1, 8, 2), (SPW + 1, 17, 20, 3)], ids=['vector', 'guarded'])
def test_garbage_outside_the_keys_changes_no_bit(dev, shape):
    c = O.case(*shape, 'both', seed=5)
    key = c['ref']['key']
    dirty = c['x'].copy()
    junk = np.where(np.arange(dirty.size).reshape(dirty.shape) % 3 == 0, np.nan, np.where(np.arange(dirty.size).reshape(dirty.shape) % 3 == 1, np.inf, -np.inf))
    dirty[~key] = junk[~key].astype(np.float32)
    assert np.isnan(dirty[~key]).any() and np.isinf(dirty[~key]).any()
    clean = _run(dev, c['x'], c['q'], c['dc'], c['lengths'], c['mask'])
    got = _run(dev, dirty, c['q'], c['dc'], c['lengths'], c['mask'])
    for k in ('out', 'lse', 'dx', 'dq'):
        assert np.array_equal(got[k], clean[k]), k
    assert not got['dx'][~key].any()


@pytest.mark.parametrize('shape', [(SPW + 1, TRIP // 2 + 1, 8, 2), (SPW + 1, 17, 20, 3)], ids=['vector', 'guarded'])
def test_a_nan_inside_the_keys_stays_in_its_sample(dev, shape):
    c = O.case(*shape, 'none', seed=6)
    bad = c['x'].copy()
    bad[1, 2, 1] = np.nan                                                    # sample 1 shares its wave with samples 0, 2 and 3
    clean = _run(dev, c['x'], c['q'], c['dc'])
    got = _run(dev, bad, c['q'], c['dc'])
    others = np.arange(shape[0]) != 1
    for k in ('out', 'lse', 'dx', 'dq'):
        assert np.array_equal(got[k][others], clean[k][others]), k
    assert np.isnan(got['out'][1]).any()


@pytest.mark.parametrize('shape', [(SPW + 1, TRIP // 2 + 1, 8, 2), (SPW + 1, 17, 20, 3)], ids=['vector', 'guarded'])
def test_dx_rows_outside_the_keys_are_zero_whatever_the_upstream_gradient_holds(dev, shape):
    """An infinite and a NaN entry in dc: the rows of dx outside the keys are written as zeros by a select, not as 0 * dc."""
    c = O.case(*shape, 'both', seed=5)
    dc = c['dc'].copy()
    dc[1, 0, 0], dc[1, 1, 1] = np.inf, np.nan
    got = _run(dev, c['x'], c['q'], dc, c['lengths'], c['mask'])
    key = c['ref']['key']
    assert (~key[1]).any() and key[1].any() and not got['dx'][~key].any()
    clean = _run(dev, c['x'], c['q'], c['dc'], c['lengths'], c['mask'])
    others = np.arange(shape[0]) != 1
    assert np.array_equal(got['dx'][others], clean['dx'][others]) and np.array_equal(got['dq'][others], clean['dq'][others])


# ---- empty and short samples ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('D', [8, 6], ids=['vector', 'guarded'])
def test_an_empty_sample_in_every_slot(dev, D):
    """An empty sample in every lane-group slot of a wave, beside lengths above L and below 0; then a batch of empty samples only."""
    B, L, H = 2 * SPW + 1, 10, 2
    rng = np.random.default_rng(41)
    x, q, dc = (rng.standard_normal(s).astype(np.float32) for s in ((B, L, D), (B, H, D), (B, H, D)))
    for slot in range(SPW):
        lengths = rng.integers(1, L + 1, B)
        lengths[slot] = 0
        lengths[(slot + 1) % SPW] = L + 5
        lengths[SPW + slot] = -3
        ref = O.run(x, q, lengths=lengths, dc=dc)
        assert not ref['key'][slot].any() and ref['key'][(slot + 1) % SPW].all() and not ref['key'][SPW + slot].any()
        _check('empty slot %d D %d' % (slot, D), _run(dev, x, q, dc, lengths=lengths), ref, 'empty')
    got = _run(dev, x, q, dc, mask=np.zeros((B, L), dtype=np.uint8))
    assert not got['out'].any() and np.isneginf(got['lse']).all() and not got['dx'].any() and not got['dq'].any()
    one = _run(dev, x[:1], q[:1], dc[:1], lengths=np.zeros(1, dtype=np.int64))                  # B = 1, the one sample empty
    assert not one['out'].any() and np.isneginf(one['lse']).all() and not one['dx'].any() and not one['dq'].any()


# ---- routes ----------------------------------------------------------------------------------------------------------------------------

def _off_by_one(a, dev, grad=False):
    """A contiguous tensor that starts one float into its buffer: off the 16-byte boundary."""
    buf = torch.zeros(a.size + 1, dtype=torch.float32, device=dev)
    buf[1:] = torch.from_numpy(np.array(a).reshape(-1)).to(dev)
    t = buf[1:].reshape(a.shape)
    assert t.is_contiguous() and t.data_ptr() % 16 != 0
    return t.requires_grad_(True) if grad else t


@pytest.mark.parametrize('which', ['user', 'query', 'dout'])
def test_misaligned_views_take_the_guarded_route(dev, which):
    B, L, D, H = SPW + 1, 17, 16, 2
    c = O.case(B, L, D, H, 'both', seed=7)
    xt = _off_by_one(c['x'], dev, True) if which == 'user' else _gpu(c['x'], dev, True)
    qt = _off_by_one(c['q'], dev, True) if which == 'query' else _gpu(c['q'], dev, True)
    dct = _off_by_one(c['dc'], dev) if which == 'dout' else _gpu(c['dc'], dev)
    out, lse = _op(xt, qt, lengths=_gpu(c['lengths'], dev), mask=_gpu(c['mask'], dev), return_lse=True)
    dx, dq = torch.autograd.grad(out, (xt, qt), dct)
    vec, guarded = _expected_route(D, H), _expected_route(D, H, vec_ok=False)
    assert vec // 100000 == 2 and guarded // 100000 == 1
    assert _route(0, B, L, D, H, xt, qt, out) == (vec if which == 'dout' else guarded)
    assert _route(1, B, L, D, H, xt, qt, out, dct, dx, dq) == guarded
    _check('misaligned %s' % which, dict(out=_np(out), lse=_np(lse), dx=_np(dx), dq=_np(dq)), c['ref'], 'misaligned')


def test_non_contiguous_inputs_are_made_contiguous(dev):
    B, L, D, H = 5, 9, 8, 2
    c = O.case(B, L, D, H, 'lengths', seed=8)
    wide = torch.zeros(B, L, 2 * D, device=dev)
    wide[:, :, :D] = _gpu(c['x'], dev)
    qT = _gpu(np.ascontiguousarray(c['q'].transpose(1, 0, 2)), dev).transpose(0, 1)
    assert not wide[:, :, :D].is_contiguous() and not qT.is_contiguous()
    out = _op(wide[:, :, :D], qT, lengths=_gpu(c['lengths'], dev))
    _hold('strided inputs out', out, c['ref']['out'], 'vector out')


# ---- frozen inputs, determinism, memory ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [(SPW + 1, TRIP // 4 + 1, 16, 3), (SPW + 1, 17, 65, 2)], ids=['vector', 'guarded'])
def test_a_frozen_input_leaves_the_other_gradient_bit_equal(dev, shape):
    c = O.case(*shape, 'both', seed=9)
    both = _run(dev, c['x'], c['q'], c['dc'], c['lengths'], c['mask'])
    only_q = _run(dev, c['x'], c['q'], c['dc'], c['lengths'], c['mask'], grad_x=False)
    only_x = _run(dev, c['x'], c['q'], c['dc'], c['lengths'], c['mask'], grad_q=False)
    assert only_q['dx'] is None and np.array_equal(only_q['dq'], both['dq'])
    assert only_x['dq'] is None and np.array_equal(only_x['dx'], both['dx'])
    assert np.array_equal(only_q['out'], both['out']) and np.array_equal(only_x['out'], both['out'])


@pytest.mark.parametrize('shape', [(2 * SPW + 1, 2 * TRIP // 4 + 2, 16, 4), (2 * SPW + 1, 19, 20, 2)], ids=['vector', 'guarded'])
def test_repeated_runs_and_graph_replay_are_bit_for_bit(dev, shape):
    c = O.case(*shape, 'both', seed=10)
    x, q, dc = _gpu(c['x'], dev, True), _gpu(c['q'], dev, True), _gpu(c['dc'], dev)
    lengths, mask = _gpu(c['lengths'].astype(np.int32), dev), _gpu(c['mask'], dev)

    def step():
        out, lse = _op(x, q, lengths=lengths, mask=mask, return_lse=True)
        return (out, lse) + torch.autograd.grad(out, (x, q), dc)
    # detached copies: a live reference to an eager step's autograd graph would keep the AccumulateGrad nodes of x and q, made under the
    # legacy default stream, alive into the capture, and ending such a capture crashes in the runtime (`bench.py --graph`)
    first = [t.detach().clone() for t in step()]
    for _ in range(3):
        assert all(torch.equal(a, b.detach()) for a, b in zip(first, step()))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    rng = np.random.default_rng(11)
    for _ in range(2):
        with torch.no_grad():                                                # new contents, same storage
            x.copy_(torch.from_numpy(rng.standard_normal(c['x'].shape).astype(np.float32)))
            dc.copy_(torch.from_numpy(rng.standard_normal(c['dc'].shape).astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, step()))


def test_peak_memory_is_the_outputs_and_the_statistic(dev):
    """B 4096, L 64, D 32, H 4: one (B, H, L) fp32 tensor would be 4 MiB.  The forward may allocate out (2 MiB), the statistic (128 KiB) and
    the (B, H) lse with its two fp64 terms; the backward dx (32 MiB) and dquery (2 MiB); each plus 64 KiB of slack."""
    B, L, D, H = 4096, 64, 32, 4
    torch.manual_seed(0)
    x = torch.randn(B, L, D, device=dev, requires_grad=True)
    q = torch.randn(B, H, D, device=dev, requires_grad=True)
    dc = torch.randn(B, H, D, device=dev)
    lengths = torch.randint(0, L + 1, (B,), device=dev, dtype=torch.int32)
    mask = (torch.rand(B, L, device=dev) > 0.2).to(torch.uint8)
    bhl = 4 * B * H * L
    for want_lse in (False, True):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = _op(x, q, lengths=lengths, mask=mask, return_lse=want_lse)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
        allowed = 4 * B * H * D + 8 * B * H + (2 * 8 + 8 + 4) * B * H * want_lse + 65536
        print('forward (lse %d): %d bytes above the inputs, allowed %d, one (B, H, L) tensor %d' % (want_lse, rise, allowed, bhl))
        assert rise <= allowed and allowed < 4 * B * H * D + bhl // 4
    out = res[0]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    dx, dq = torch.autograd.grad(out, (x, q), dc)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    allowed = 4 * B * L * D + 4 * B * H * D + 65536
    print('backward: %d bytes above the inputs, allowed %d' % (rise, allowed))
    assert rise <= allowed and dx.shape == x.shape and dq.shape == q.shape


# ---- the layer -------------------------------------------------------------------------------------------------------------------------

def _layer_case(D, seed):
    rng = np.random.default_rng(seed)
    B, L, Dq, H, d = 7, 11, 5, 2, 3
    x, doc, g = (rng.standard_normal(s).astype(np.float32) for s in ((B, L, D), (B, Dq), (B, H * d)))
    W = [(rng.standard_normal(s) / math.sqrt(s[0])).astype(np.float32) for s in ((Dq, H * d), (D, H * d), (D, H * d))]
    lengths = rng.integers(1, L + 1, B)
    lengths[0], lengths[2], lengths[B - 1] = L, 0, 0
    mask = (rng.random((B, L)) >= 0.2).astype(np.uint8)
    mask[0] = 1
    return x, doc, g, W, lengths, mask, H, d


@pytest.mark.parametrize('scaling', [True, False])
@pytest.mark.parametrize('D', [8, 6], ids=['vector', 'guarded'])
def test_layer_matches_the_oracle(dev, D, scaling):
    from rec_now_amd.layers import TargetAttentionLayer
    x, doc, g, W, lengths, mask, H, d = _layer_case(D, 51)
    ref = O.run_layer(x, doc, *W, H, scaling, lengths, mask, g)
    lay = TargetAttentionLayer(H, d, scaling=scaling)
    lay._build_device = dev
    lay.build((x.shape, doc.shape))
    lay.set_weights_by_name(dict(zip(('W_query', 'W_key', 'W_value'), W)))
    xt, dt = _gpu(x, dev, True), _gpu(doc, dev, True)
    out = lay(xt, dt, lengths=_gpu(lengths, dev), mask=_gpu(mask, dev))
    grads = torch.autograd.grad(out, [xt, dt, lay.W_query, lay.W_key, lay.W_value], _gpu(g, dev))
    assert out.shape == ref['out'].shape and not _np(out)[2].any() and not _np(out)[-1].any()      # a sample without a key: a zero row
    _hold('layer out', out, ref['out'], 'layer out')
    _hold('layer dx', grads[0], ref['dx'], 'layer dx')
    _hold('layer ddoc', grads[1], ref['ddoc'], 'layer ddoc')
    for name, got in zip(('dWq', 'dWk', 'dWv'), grads[2:]):
        _hold('layer ' + name, got, ref[name], 'layer ' + name, O.tensorfrac)


def test_layer_and_a_dense_head_match_fp64_autograd(dev):
    """TargetAttentionLayer -> MultiDenseLayer with empty samples in the batch: the output, dx, ddoc and every parameter gradient against fp64
    autograd of the unfolded composition (every position projected, masked_fill + softmax, empty rows patched to zero)."""
    import dense_ref as R
    from rec_now_amd.layers import TargetAttentionLayer
    from rec_now_amd.layers.multi_dense_layer import MultiDenseLayer
    torch.manual_seed(7)
    x, doc, _, W, lengths, mask, H, d = _layer_case(16, 52)
    B, L, D = x.shape
    rng = np.random.default_rng(53)
    lay, head = TargetAttentionLayer(H, d), MultiDenseLayer(4, 1)
    xt, dt = _gpu(x, dev, True), _gpu(doc, dev, True)
    gy = _gpu(rng.standard_normal((B, 4)).astype(np.float32), dev)
    y = head(lay(xt, dt, lengths=_gpu(lengths, dev), mask=_gpu(mask, dev))).reshape(B, 4)
    params = dict(lay.named_weights())
    params.update({'head/kernel': head.kernel, 'head/bias': head.bias})
    grads = torch.autograd.grad(y, [xt, dt] + list(params.values()), gy)
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in params.items()}
    x64, d64 = (torch.from_numpy(a).double().requires_grad_(True) for a in (x, doc))
    key = torch.from_numpy(O.keys_of(B, L, lengths, mask))
    Q = (d64 @ p64['W_query']).reshape(B, H, d)
    K, V = ((x64 @ p64[n]).reshape(B, L, H, d) for n in ('W_key', 'W_value'))
    s = (torch.einsum('bhc,blhc->bhl', Q, K) / math.sqrt(d)).masked_fill(~key[:, None, :], float('-inf'))
    a = torch.where(key.any(1)[:, None, None], torch.softmax(s, -1), torch.zeros_like(s))
    z = torch.einsum('bhl,blhc->bhc', a, V).reshape(B, H * d)
    y64 = R.multi_dense_layer(z, p64['head/kernel'], p64['head/bias']).reshape(B, 4)
    assert not bool(key[2].any()) and not bool(key[-1].any())
    _hold('module out', y, y64.detach().numpy(), 'module out')
    g64 = torch.autograd.grad(y64, [x64, d64] + list(p64.values()), gy.cpu().double())
    for name, got, want in zip(['x', 'doc'] + list(params), grads, g64):
        _hold('module d ' + name, got, want.numpy(), 'module d ' + name, O.rowfrac if name in ('x', 'doc') else O.tensorfrac)


def test_zz_report_the_worst_fractions():
    """Last in the file: the largest fraction of its bound seen per tensor by the tests above (printed; the bounds are asserted there)."""
    for what in sorted(WORST):
        print('worst %-24s %.3f of the bound' % (what, WORST[what]))
    assert all(v <= 1.0 for v in WORST.values())
