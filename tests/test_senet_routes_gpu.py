"""Every path through recnow_senet_fused_fwd / _bwd and recnow_senet_squeeze / _scale_fwd / _scale_bwd_w / _scale_bwd_x (tests/_senet_routes.py), through
the C ABI on guard-banded buffers (tests/_guard.py) and through SENETLayer.  Each row checks:
  1. route: recnow_senet_fused_route / _grid (recnow_senet_route / _grid) answer the row's codes and the mirror's grids for the very pointers the call
     is made with; the backward's grid is min(ceil(B / 4), 2048) or a multiple of 256 below it, and the passes a row made are stated from it;
  2. the C entries on NaN-filled outputs inside sentinel bands -- sq_save, h_save and w_save included, each compared per entry; the backward is fed
     what the forward saved;
  3. fp64: every output entry against oracle/dense_ref.senet_layer under fp64 autograd (what the oracle does not return -- sq, h, w, and the four
     unfused entries on their own inputs -- against the closed form the CPU test holds to the oracle), at 1e-5 of the cancellation-free magnitude of
     what THAT entry summed; a scale of 0 demands an error of 0; relu pre-activations keep KINK of their magnitude from 0 in fp64;
  4. census: on integer data every output equals the fp64 value bit for bit, the sign of a zero included;
  5. untouched memory: no NaN left in an output, every band around inputs, outputs and the workspace intact (the band starts at row B), the inputs
     unchanged;
  6. the public layer on the same data, weights set by name, with the same bounds and the same census (a misaligned out and one bias of two are
     C ABI only);
  7. on the two-pass rows the backward runs twice and gives the same bits (csrc/senet_fused.hip: the weight gradients are deterministic);
  8. the alignment rows: the layer is handed a field / an upstream gradient that is a contiguous view one float into a larger buffer, and the
     pointers that reach the C calls are on 16-byte boundaries -- or the tile route is what ran.  No float4 kernel is run on a misaligned pointer.
uni_two_pass holds 67 M floats a tensor: census only, expected values formed in fp32 numpy, compared on the device; it takes some ten seconds, most of
them host arithmetic and uploads.  B = 0, null pointers, a short workspace and total = 12288 are tests of their own below: nothing is launched, nothing is written.
The worst margin of every row is printed; the module's margin_report fixture prints the worst per output after the last test."""
import ctypes

import numpy as np
import pytest
import torch

import _senet_census as C
import _senet_routes as T
from _guard import Buf

pytestmark = pytest.mark.gpu
USED = {}
PASSES = {}
ROWS = [r for r in T.ROUTES if not r['census_only']]


@pytest.fixture(scope='module', autouse=True)
def margin_report():
    """after the last test of this module: the largest fraction of its bound that any row which ran used, per output; the passes observed"""
    yield
    for key in sorted({k for m in USED.values() for k in m}):
        sel = {n: m[key] for n, m in USED.items() if key in m}
        worst = max(sel, key=sel.get)
        print('senet.%s: at most %.4f of the bound (%s)' % (key, sel[worst], worst))
    for name, p in sorted(PASSES.items()):
        print('passes %s: %s' % (name, p))


def P(q):
    return ctypes.c_void_p(q.ptr) if q is not None else None


def _ptrs(dev, bufs):
    return torch.tensor([b.ptr for b in bufs], dtype=torch.int64, device=dev)


def _settle(name, bufs, ins, outs):
    """after the calls: bands intact, no NaN left in an output, inputs unchanged"""
    torch.cuda.synchronize()
    for k, q in bufs.items():
        for i, b in enumerate(q if isinstance(q, list) else [q]):
            assert b is None or b.damaged() == 0, '%s: %d guard words of %s[%d] changed' % (name, b.damaged(), k, i)
    for k, v in outs.items():
        assert not np.isnan(C._flat(v)).any(), '%s: NaN left in %s' % (name, k)
    for k, (q, v) in ins.items():
        assert C.same_bits(q.get(np.shape(v)), v), '%s: the input %s was written' % (name, k)
    return outs


def run_c_fused(dev, r, d, acts):
    """recnow_senet_fused_fwd / _bwd of row r on guard-banded buffers, after asking the route queries about these very pointers"""
    from rec_now_amd import _lib
    lib = _lib.load()
    B, F, D, M = r['B'], r['F'], r['D'], r['M']
    st = _lib.stream()
    xs = [Buf(dev, B * D, d['x'][f]) for f in range(F)]
    dxs = [Buf(dev, B * D) for _ in range(F)]
    xp, dxp = _ptrs(dev, xs), _ptrs(dev, dxs)
    W1, W2 = Buf(dev, F * M, d['W1']), Buf(dev, M * F, d['W2'])
    b1 = Buf(dev, M, d['b1']) if d['b1'] is not None else None
    b2 = Buf(dev, F, d['b2']) if d['b2'] is not None else None
    out = Buf(dev, B * F * D, lead=r['out_lead'])
    sq, h, w = Buf(dev, B * F), Buf(dev, B * M), Buf(dev, B * F)
    dout = Buf(dev, B * F * D, d['dout'])
    dW1, dW2 = Buf(dev, F * M), Buf(dev, M * F)
    db1, db2 = (Buf(dev, M) if b1 is not None else None), (Buf(dev, F) if b2 is not None else None)
    nws = lib.recnow_senet_fused_workspace_bytes(B, F, M)
    assert nws % 4 == 0
    ws = Buf(dev, nws // 4)
    assert all(q.ptr % 16 == 0 for q in xs + dxs + [dout]) and out.ptr % 16 == 4 * r['out_lead']
    mis = int(out.ptr % 16 != 0)
    # 1. the routes and the grids
    assert lib.recnow_senet_fused_route(0, B, F, D, M, mis) == r['fwd'], 'forward route'
    assert lib.recnow_senet_fused_route(1, B, F, D, M, 0) == r['bwd'], 'backward route'
    assert lib.recnow_senet_fused_grid(0, B, F, D, M, mis) == T.fused_grid(0, B, F, D, M, mis)
    gb = lib.recnow_senet_fused_grid(1, B, F, D, M, 0)
    cap = min(-(-B // 4), 2048)
    assert gb == cap or (0 < gb < cap and gb % 256 == 0), 'backward grid %d of %d' % (gb, cap)
    geo = T.geometry(r, bwd_grid=gb)
    PASSES[r['name']] = 'forward %d (grid %d), backward %d (grid %d)' % (geo['f']['passes'], geo['f']['grid'], geo['b']['passes'], gb)
    if 'two_pass' in r['name']:
        assert geo['f']['passes'] == 2 and geo['b']['passes'] >= 2 and B % geo['b']['stride'] and B % geo['f']['stride']
    # 2. the calls
    _lib.call('recnow_senet_fused_fwd', _lib.ptr(xp), F, D, B, P(W1), P(b1), P(W2), P(b2), M, acts[0], acts[1], P(out), P(sq), P(h), P(w), st)
    torch.cuda.synchronize()
    outs = dict(out=out.get((B, F * D)), sq=sq.get((B, F)), h=h.get((B, M)), w=w.get((B, F)))

    def backward():
        for q in dxs + [dW1, dW2, db1, db2, ws]:
            if q is not None:
                q.nan()
        _lib.call('recnow_senet_fused_bwd', _lib.ptr(xp), _lib.ptr(dxp), F, D, B, P(W1), P(W2), M, acts[0], acts[1], P(dout), P(sq), P(h), P(w), P(dW1), P(db1),
                  P(dW2), P(db2), P(ws), nws, st)
        torch.cuda.synchronize()
        res = dict(dx=[q.get((B, D)) for q in dxs], dW1=dW1.get((F, M)), dW2=dW2.get((M, F)))
        if db1 is not None:
            res['db1'] = db1.get((M,))
        if db2 is not None:
            res['db2'] = db2.get((F,))
        return res

    back = backward()
    if 'two_pass' in r['name']:                                   # 7. deterministic weight gradients
        again = backward()
        for k in back:
            assert C.bits_equal(back[k], again[k]), '%s: %s differs between two runs of the backward' % (r['name'], k)
    outs.update(back)
    ins = {'x[%d]' % f: (xs[f], d['x'][f]) for f in range(F)}
    ins.update(W1=(W1, d['W1']), W2=(W2, d['W2']), dout=(dout, d['dout']), sq_save=(sq, outs['sq']), h_save=(h, outs['h']), w_save=(w, outs['w']))
    ins.update({k: (q, d[k]) for k, q in (('b1', b1), ('b2', b2)) if q is not None})
    return _settle(r['name'], dict(x=xs, dx=dxs, W1=W1, W2=W2, b1=b1, b2=b2, out=out, sq=sq, h=h, w=w, dout=dout, dW1=dW1, dW2=dW2, db1=db1, db2=db2, ws=ws), ins, outs)


def run_c_unfused(dev, r, d):
    """the four unfused entries of row r on guard-banded buffers (w, dout and dsq are inputs there)"""
    from rec_now_amd import _lib
    lib = _lib.load()
    B, F, dims, ud = r['B'], r['F'], r['dims'], r['ud']
    total = sum(dims)
    st = _lib.stream()
    offs = [int(v) for v in np.concatenate([[0], np.cumsum(dims)[:-1]])]
    dd, oo = torch.tensor(dims, dtype=torch.int32, device=dev), torch.tensor(offs, dtype=torch.int32, device=dev)
    xs = [Buf(dev, B * n, d['x'][f]) for f, n in enumerate(dims)]
    dxs = [Buf(dev, B * n) for n in dims]
    xp, dxp = _ptrs(dev, xs), _ptrs(dev, dxs)
    w, dout, dsq = Buf(dev, B * F, d['w']), Buf(dev, B * total, d['dout']), Buf(dev, B * F, d['dsq'])
    sq, out, dw = Buf(dev, B * F), Buf(dev, B * total), Buf(dev, B * F)
    assert all(q.ptr % 16 == 0 for q in xs + dxs + [dout, out])
    for mode in (T.SQUEEZE, T.SCALE, T.DW, T.DX):
        assert lib.recnow_senet_route(mode, B, F, total, ud) == r['code'], 'route of mode %d' % mode
        assert lib.recnow_senet_grid(mode, B, F, total, ud) == T.senet_grid(mode, B, F, total, ud)
    e = T.geometry(r)['u']
    PASSES[r['name']] = '%d (grid %d)' % (e['passes'], e['grid'])
    if 'two_pass' in r['name']:
        assert e['passes'] == 2
    _lib.call('recnow_senet_squeeze', _lib.ptr(xp), _lib.ptr(dd), _lib.ptr(oo), F, total, B, P(sq), ud, st)
    _lib.call('recnow_senet_scale_fwd', _lib.ptr(xp), _lib.ptr(dd), _lib.ptr(oo), F, total, B, P(w), P(out), ud, st)
    _lib.call('recnow_senet_scale_bwd_w', _lib.ptr(xp), _lib.ptr(dd), _lib.ptr(oo), F, total, B, P(dout), P(dw), ud, st)
    _lib.call('recnow_senet_scale_bwd_x', _lib.ptr(dxp), _lib.ptr(dd), _lib.ptr(oo), F, total, B, P(w), P(dout), P(dsq), ud, st)
    torch.cuda.synchronize()
    outs = dict(e_sq=sq.get((B, F)), e_out=out.get((B, total)), e_dw=dw.get((B, F)), e_dx=[q.get((B, n)) for q, n in zip(dxs, dims)])
    ins = {'x[%d]' % f: (xs[f], d['x'][f]) for f in range(F)}
    ins.update(w=(w, d['w']), dout=(dout, d['dout']), dsq=(dsq, d['dsq']))
    return _settle(r['name'], dict(x=xs, dx=dxs, w=w, dout=dout, dsq=dsq, sq=sq, out=out, dw=dw), ins, outs)


def _dev_tensor(dev, a, view, grad=True):
    """a on the device (a leaf that wants a gradient); view: a contiguous view that starts one float into a larger buffer"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not view:
        return t.to(dev).requires_grad_(grad)
    buf = torch.zeros(t.numel() + 8, dtype=torch.float32, device=dev)
    buf[1:1 + t.numel()] = t.reshape(-1).to(dev)
    v = buf[1:1 + t.numel()].view(t.shape).detach().requires_grad_(grad)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


class _Spy:
    """wraps _lib.call and _lib.ptr_array while the layer runs: which entries were called with which pointers"""

    def __init__(self, lib_mod):
        self.m, self.calls, self.arrays = lib_mod, [], []

    def __enter__(self):
        self.call, self.ptr_array = self.m.call, self.m.ptr_array

        def call(name, *args):
            self.calls.append((name, [a.value if isinstance(a, ctypes.c_void_p) else a for a in args]))
            return self.call(name, *args)

        def ptr_array(tensors, device):
            self.arrays.append([t.data_ptr() for t in tensors])
            return self.ptr_array(tensors, device)

        self.m.call, self.m.ptr_array = call, ptr_array
        return self

    def __exit__(self, *exc):
        self.m.call, self.m.ptr_array = self.call, self.ptr_array

    def args(self, name):
        got = [a for n, a in self.calls if n == name]
        assert len(got) == 1, (name, [n for n, _ in self.calls])
        return got[0]


def run_layer(dev, r, d, acts):
    """forward and backward of row r through SENETLayer, weights set by name; the pointers that reach the C calls are inspected (8.)"""
    from rec_now_amd import _lib
    from rec_now_amd.layers.senet_layer import SENETLayer
    lib = _lib.load()
    B, F, dims, M = r['B'], r['F'], r['dims'], r['M']
    total = sum(dims)
    layer = SENETLayer(M / F, activation_inner=T.ACT_NAMES[acts[0]], activation_outer=T.ACT_NAMES[acts[1]], use_bias=bool(r['b1']))
    xs = [_dev_tensor(dev, d['x'][f], r['view'] == 'field' and f == min(1, F - 1)) for f in range(F)]
    layer([x.detach()[:1] for x in xs])                          # builds
    assert layer.middle_dim == M
    name = layer.name
    vals = {f'{name}/senet/dense_0/kernel': d['W1'], f'{name}/senet/dense_1/kernel': d['W2']}
    if r['b1']:
        vals.update({f'{name}/senet/dense_0/bias': d['b1'], f'{name}/senet/dense_1/bias': d['b2']})
    layer.set_weights_by_name(vals)
    wts = layer.named_weights()
    params = [wts[k] for k in vals]
    up = _dev_tensor(dev, d['dout'], r['view'] == 'dout', grad=False)
    with _Spy(_lib) as spy:
        out = layer(xs)
        grads = torch.autograd.grad(out, xs + params, up)
    assert out.data_ptr() % 16 == 0
    names = [n for n, _ in spy.calls]
    if r['kind'] == 'fused':
        assert 'recnow_senet_squeeze' not in names
        fa, ba = spy.args('recnow_senet_fused_fwd'), spy.args('recnow_senet_fused_bwd')
        fields = next(a for a in spy.arrays if len(a) == F)
        assert all(p % 16 == 0 for p in fields), 'a misaligned field reached the fused kernels'
        assert fa[11] % 16 == 0 and ba[10] % 16 == 0, 'out / dout of the fused kernels off a 16-byte boundary'
        assert lib.recnow_senet_fused_route(0, B, F, r['D'], M, 0) == r['fwd'] and (fa[1], fa[2], fa[3], fa[8]) == (F, r['D'], B, M)
    else:
        assert 'recnow_senet_fused_fwd' not in names
        s, f, bw_, bx = (spy.args('recnow_senet_' + n) for n in ('squeeze', 'scale_fwd', 'scale_bwd_w', 'scale_bwd_x'))
        ud = s[7]
        assert f[8] == ud and bw_[8] == ud and bx[9] == ud and lib.recnow_senet_route(0, B, F, total, ud) == r['code'], 'the layer took another route'
        if ud:                                                    # the float4 route: every pointer it reads by float4 is aligned
            fields = next(a for a in spy.arrays if len(a) == F)
            assert all(p % 16 == 0 for p in fields) and bw_[6] % 16 == 0 and bx[7] % 16 == 0 and f[7] % 16 == 0
        else:
            assert r['code'] // 100000 == T.SENET_TILE
    if r['view'] == 'dout':
        assert up.data_ptr() % 16 == 4                           # what autograd handed the backward was the misaligned view
    g = [v.detach().cpu().numpy() for v in grads]
    res = dict(out=out.detach().cpu().numpy(), dx=g[:F], dW1=g[F], dW2=g[F + 1])
    if r['b1']:
        res.update(db1=g[F + 2], db2=g[F + 3])
    return res


def _bits(name, tag, keys, got, want):
    for k in keys:
        a, e = C._flat(got[k]).astype(np.float32).reshape(-1), C._flat(want[k]).astype(np.float32).reshape(-1)
        assert a.shape == e.shape
        bad = np.flatnonzero(a.view(np.int32) != e.view(np.int32))
        assert bad.size == 0, '%s census (%s): %d of %d words of %s differ from the exact value, first flat %d: %r vs %r' % (
            name, tag, bad.size, a.size, k, bad[0], a[bad[0]], e[bad[0]])


@pytest.mark.parametrize('r', ROWS, ids=[r['name'] for r in ROWS])
def test_senet_route(dev, r):
    fused = r['kind'] == 'fused'
    # random data against fp64, entry by entry
    d = C.random_data(r)
    lo = C.kink_clearance(d, r['acts'])
    assert lo >= C.KINK, 'a relu pre-activation %.3g of its magnitude from 0' % lo
    closed = C.model(r, d, scales=True)
    ref = dict(closed)
    ref.update(C.oracle(d, r['acts']))                           # out and every gradient: fp64 autograd of the oracle; sq, h, w: the closed form
    worst = {}

    def hold(tag, keys, got, want, sc):
        m = C.margins(keys, got, want, sc)
        print('%s (%s): fraction of the bound used %s' % (r['name'], tag, '  '.join('%s %.4f' % kv for kv in sorted(m.items()))))
        for k, v in m.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 1.0, '%s (%s): %s is %.3g times the bound (1e-5 of the entry\'s cancellation-free scale)' % (r['name'], tag, k, v)

    if fused:
        got = run_c_fused(dev, r, d, r['acts'])
        assert set(got) == set(C.outputs(r))
        hold('C', C.outputs(r), got, ref, closed)
    else:
        ent = C.entry(r, d, scales=True)
        got = run_c_unfused(dev, r, d)
        assert set(got) == set(C.ENTRY_OUT)
        hold('C', C.ENTRY_OUT, got, ent, ent)
    if r['layer']:
        hold('layer', C.outputs(r, 'layer'), run_layer(dev, r, d, r['acts']), ref, closed)
    USED[r['name']] = worst
    # census data, bit for bit
    c, _ = C.make(r)
    acts = C.census_acts(r['acts'])
    want = C.model(r, c, acts)
    if fused:
        _bits(r['name'], 'C', C.outputs(r), run_c_fused(dev, r, c, acts), want)
    else:
        _bits(r['name'], 'C', C.ENTRY_OUT, run_c_unfused(dev, r, c), C.entry(r, c))
    if r['layer'] and r.get('layer_census', True):
        _bits(r['name'], 'layer', C.outputs(r, 'layer'), run_layer(dev, r, c, acts), want)


def test_uniform_two_pass_census(dev):
    """uni_two_pass: the second, ragged pass of k_senet_uniform in all four modes.  67 M floats a tensor: census only -- integer data whose sums stay
    below 2^24 by arithmetic (tests/test_senet_census_cpu.py), expected values formed in fp32 numpy (exact in any order), compared on the device.
    This row takes longer than a few seconds: some ten, most of them host arithmetic and uploads."""
    from rec_now_amd import _lib
    lib = _lib.load()
    r = T.BY_NAME['uni_two_pass']
    B, F, dims, ud = r['B'], r['F'], r['dims'], r['ud']
    total, D = sum(dims), dims[0]
    e = T.geometry(r)['u']
    assert e['passes'] == 2 and e['items'] - e['per'] == 16 and lib.recnow_senet_grid(0, B, F, total, ud) == 16384 == e['grid']
    PASSES[r['name']] = '%d (grid %d)' % (e['passes'], e['grid'])
    d, _ = C.make(r)
    want = C.entries(d, np.float32)
    assert all(np.asarray(v if not isinstance(v, list) else v[0]).dtype == np.float32 for v in want.values())
    st = _lib.stream()
    xs = [Buf(dev, B * D, d['x'][f]) for f in range(F)]
    xp = _ptrs(dev, xs)
    dd, oo = torch.tensor(dims, dtype=torch.int32, device=dev), torch.tensor([0, D], dtype=torch.int32, device=dev)
    w, dsq = Buf(dev, B * F, d['w']), Buf(dev, B * F, d['dsq'])
    sq, dw = Buf(dev, B * F), Buf(dev, B * F)

    def same(q, a, what):
        e32 = torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).to(dev)
        bad = int((q.body.view(torch.int32) != e32.view(torch.int32)).sum())
        assert bad == 0 and q.damaged() == 0, '%s: %d words differ, %d guard words changed' % (what, bad, q.damaged())

    for mode in (T.SQUEEZE, T.SCALE, T.DW, T.DX):
        assert lib.recnow_senet_route(mode, B, F, total, ud) == r['code']
    _lib.call('recnow_senet_squeeze', _lib.ptr(xp), _lib.ptr(dd), _lib.ptr(oo), F, total, B, P(sq), ud, st)
    same(sq, want['e_sq'], 'squeeze')
    out = Buf(dev, B * total)
    _lib.call('recnow_senet_scale_fwd', _lib.ptr(xp), _lib.ptr(dd), _lib.ptr(oo), F, total, B, P(w), P(out), ud, st)
    same(out, want['e_out'], 'scale_fwd')
    del out
    dout = Buf(dev, B * total, d['dout'])
    _lib.call('recnow_senet_scale_bwd_w', _lib.ptr(xp), _lib.ptr(dd), _lib.ptr(oo), F, total, B, P(dout), P(dw), ud, st)
    same(dw, want['e_dw'], 'scale_bwd_w')
    dxs = [Buf(dev, B * D) for _ in range(F)]
    dxp = _ptrs(dev, dxs)
    _lib.call('recnow_senet_scale_bwd_x', _lib.ptr(dxp), _lib.ptr(dd), _lib.ptr(oo), F, total, B, P(w), P(dout), P(dsq), ud, st)
    for f in range(F):
        same(dxs[f], want['e_dx'][f], 'scale_bwd_x field %d' % f)
    for q, v, k in [(xs[0], d['x'][0], 'x[0]'), (xs[1], d['x'][1], 'x[1]'), (w, d['w'], 'w'), (dsq, d['dsq'], 'dsq'), (dout, d['dout'], 'dout')]:
        same(q, v, 'the input ' + k)


# ---- calls that launch nothing ----------------------------------------------------------------------------------------------------------------------------
def _small(dev, B=5, F=3, D=8, M=2):
    xs = [Buf(dev, B * D, np.ones((B, D), np.float32)) for _ in range(F)]
    dxs = [Buf(dev, B * D) for _ in range(F)]
    return dict(xs=xs, dxs=dxs, xp=_ptrs(dev, xs), dxp=_ptrs(dev, dxs), W1=Buf(dev, F * M, np.ones(F * M)), W2=Buf(dev, F * M, np.ones(F * M)),
                out=Buf(dev, B * F * D), sq=Buf(dev, B * F), h=Buf(dev, B * M), w=Buf(dev, B * F), dout=Buf(dev, B * F * D, np.ones(B * F * D)),
                dW1=Buf(dev, F * M), dW2=Buf(dev, F * M), db1=Buf(dev, M), db2=Buf(dev, F))


def _all_untouched(bufs):
    torch.cuda.synchronize()
    return all(q.untouched() and q.damaged() == 0 for q in bufs)


def test_empty_batch_writes_only_the_zeroed_weight_gradients(dev):
    """B = 0 on every entry: RECNOW_OK; the fused backward zeroes dW1, dW2, db1, db2; nothing else is written"""
    from rec_now_amd import _lib
    lib = _lib.load()
    F, D, M = 3, 8, 2
    s = _small(dev)
    st = _lib.stream()
    dd, oo = torch.tensor([D] * F, dtype=torch.int32, device=dev), torch.tensor([0, D, 2 * D], dtype=torch.int32, device=dev)
    ws = Buf(dev, 1024)
    outs = [s['out'], s['sq'], s['h'], s['w']] + s['dxs']
    assert lib.recnow_senet_fused_fwd(_lib.ptr(s['xp']), F, D, 0, P(s['W1']), None, P(s['W2']), None, M, 1, 3, P(s['out']), P(s['sq']), P(s['h']), P(s['w']), st) == 0
    for ud in (0, D):
        assert lib.recnow_senet_squeeze(_lib.ptr(s['xp']), _lib.ptr(dd), _lib.ptr(oo), F, F * D, 0, P(s['sq']), ud, st) == 0
        assert lib.recnow_senet_scale_fwd(_lib.ptr(s['xp']), _lib.ptr(dd), _lib.ptr(oo), F, F * D, 0, P(s['w']), P(s['out']), ud, st) == 0
        assert lib.recnow_senet_scale_bwd_w(_lib.ptr(s['xp']), _lib.ptr(dd), _lib.ptr(oo), F, F * D, 0, P(s['dout']), P(s['sq']), ud, st) == 0
        assert lib.recnow_senet_scale_bwd_x(_lib.ptr(s['dxp']), _lib.ptr(dd), _lib.ptr(oo), F, F * D, 0, P(s['w']), P(s['dout']), P(s['sq']), ud, st) == 0
    assert _all_untouched(outs + [s['dW1'], s['dW2'], s['db1'], s['db2']])
    assert lib.recnow_senet_fused_bwd(_lib.ptr(s['xp']), _lib.ptr(s['dxp']), F, D, 0, P(s['W1']), P(s['W2']), M, 1, 3, P(s['dout']), P(s['sq']), P(s['h']), P(s['w']),
                                      P(s['dW1']), P(s['db1']), P(s['dW2']), P(s['db2']), P(ws), 4096, st) == 0
    torch.cuda.synchronize()
    for k, n in (('dW1', F * M), ('dW2', F * M), ('db1', M), ('db2', F)):
        assert C.same_bits(s[k].get((n,)), np.zeros(n)) and s[k].damaged() == 0, k
    assert _all_untouched(outs + [ws])
    # db1 / db2 NULL at B = 0
    s['dW1'].nan()
    assert lib.recnow_senet_fused_bwd(_lib.ptr(s['xp']), _lib.ptr(s['dxp']), F, D, 0, P(s['W1']), P(s['W2']), M, 1, 3, P(s['dout']), P(s['sq']), P(s['h']), P(s['w']),
                                      P(s['dW1']), None, P(s['dW2']), None, P(ws), 4096, st) == 0
    torch.cuda.synchronize()
    assert C.same_bits(s['dW1'].get((F * M,)), np.zeros(F * M))


def test_refused_calls_launch_nothing(dev):
    """a workspace one byte short: RECNOW_EWORKSPACE; a null required pointer: RECNOW_EINVAL; total = 12288 without the promise: RECNOW_EUNSUPPORTED.
    Every output keeps the NaN it was filled with."""
    from rec_now_amd import _lib
    lib = _lib.load()
    B, F, D, M = 5, 3, 8, 2
    s = _small(dev)
    st = _lib.stream()
    nws = lib.recnow_senet_fused_workspace_bytes(B, F, M)
    ws = Buf(dev, nws // 4)
    outs = [s['out'], s['sq'], s['h'], s['w'], s['dW1'], s['dW2'], s['db1'], s['db2'], ws] + s['dxs']
    sv = [Buf(dev, B * F, np.ones(B * F)), Buf(dev, B * M, np.ones(B * M)), Buf(dev, B * F, np.ones(B * F))]

    def bwd(**kw):
        a = dict(xp=_lib.ptr(s['xp']), dxp=_lib.ptr(s['dxp']), W1=P(s['W1']), W2=P(s['W2']), dout=P(s['dout']), sq=P(sv[0]), h=P(sv[1]), w=P(sv[2]), dW1=P(s['dW1']),
                 dW2=P(s['dW2']), ws=P(ws), n=nws)
        a.update(kw)
        return lib.recnow_senet_fused_bwd(a['xp'], a['dxp'], F, D, B, a['W1'], a['W2'], M, 1, 3, a['dout'], a['sq'], a['h'], a['w'], a['dW1'], P(s['db1']), a['dW2'],
                                          P(s['db2']), a['ws'], a['n'], st)

    assert bwd(n=nws - 1) == -2
    for k in ('xp', 'dxp', 'W1', 'W2', 'dout', 'sq', 'h', 'w', 'dW1', 'dW2', 'ws'):
        assert bwd(**{k: None}) == -1, k

    def fwd(**kw):
        a = dict(xp=_lib.ptr(s['xp']), W1=P(s['W1']), W2=P(s['W2']), out=P(s['out']), sq=P(s['sq']), h=P(s['h']), w=P(s['w']))
        a.update(kw)
        return lib.recnow_senet_fused_fwd(a['xp'], F, D, B, a['W1'], None, a['W2'], None, M, 1, 3, a['out'], a['sq'], a['h'], a['w'], st)

    for k in ('xp', 'W1', 'W2', 'out', 'sq', 'h', 'w'):
        assert fwd(**{k: None}) == -1, k
    assert lib.recnow_senet_fused_fwd(_lib.ptr(s['xp']), 65, 4, B, P(s['W1']), None, P(s['W2']), None, M, 1, 3, P(s['out']), P(s['sq']), P(s['h']), P(s['w']), st) == -3
    dd, oo = torch.tensor([D] * F, dtype=torch.int32, device=dev), torch.tensor([0, D, 2 * D], dtype=torch.int32, device=dev)
    xp, dp, op = _lib.ptr(s['xp']), _lib.ptr(dd), _lib.ptr(oo)
    assert lib.recnow_senet_squeeze(None, dp, op, F, F * D, B, P(s['sq']), 0, st) == -1 and lib.recnow_senet_squeeze(xp, dp, op, F, F * D, B, None, D, st) == -1
    assert lib.recnow_senet_scale_fwd(xp, dp, op, F, F * D, B, None, P(s['out']), 0, st) == -1 and lib.recnow_senet_scale_bwd_w(xp, None, op, F, F * D, B, P(s['dout']), P(s['sq']), 0, st) == -1
    assert lib.recnow_senet_scale_bwd_x(_lib.ptr(s['dxp']), dp, op, F, F * D, B, P(s['w']), P(s['dout']), None, 0, st) == -1
    # total = 12288: one concatenated row no longer fits in LDS
    big = T.TOTAL_UNSUPPORTED
    assert lib.recnow_senet_route(0, 3, len(big), sum(big), 0) == T.EUNSUPPORTED
    bx = [Buf(dev, 3 * n, np.ones(3 * n)) for n in big]
    bdx = [Buf(dev, 3 * n) for n in big]
    bdd, boo = torch.tensor(big, dtype=torch.int32, device=dev), torch.tensor([0, big[0]], dtype=torch.int32, device=dev)
    bsq, bout, bw_, bdout = Buf(dev, 6), Buf(dev, 3 * sum(big)), Buf(dev, 6, np.ones(6)), Buf(dev, 3 * sum(big), np.ones(3 * sum(big)))
    bxp, bdxp = _ptrs(dev, bx), _ptrs(dev, bdx)
    assert lib.recnow_senet_squeeze(_lib.ptr(bxp), _lib.ptr(bdd), _lib.ptr(boo), 2, sum(big), 3, P(bsq), 0, st) == -3
    assert lib.recnow_senet_scale_fwd(_lib.ptr(bxp), _lib.ptr(bdd), _lib.ptr(boo), 2, sum(big), 3, P(bw_), P(bout), 0, st) == -3
    assert lib.recnow_senet_scale_bwd_w(_lib.ptr(bxp), _lib.ptr(bdd), _lib.ptr(boo), 2, sum(big), 3, P(bdout), P(bsq), 0, st) == -3
    assert lib.recnow_senet_scale_bwd_x(_lib.ptr(bdxp), _lib.ptr(bdd), _lib.ptr(boo), 2, sum(big), 3, P(bw_), P(bdout), P(bw_), 0, st) == -3
    assert _all_untouched(outs + [bsq, bout] + bdx)
