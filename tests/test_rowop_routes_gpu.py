"""Every path through recnow_fm_fwd / _bwd, recnow_inner_pnn_fwd / _bwd and recnow_attention_dot_fwd / _bwd (tests/_rowop_routes.py), through the C ABI
on guard-banded buffers (tests/_guard.py) and through FMLayer, InnerPNNLayer and attention_by_dot_product.  Each row checks:
  1. route: the route query answers the row's codes for the very pointers the call is made with;
  2. public entry points: forward and backward through the layer (rows only the C ABI reaches -- S = NULL, out / dout off a 16-byte boundary -- make the
     C call alone; where the backward tile of InnerPNN does not fit the layer's backward must raise);
  3. fp64: every output entry against oracle/dense_ref under fp64 autograd, at 1e-5 of the cancellation-free magnitude of what THAT entry summed
     (_rowop_census margins(): not the maximum of the tensor; the scales come from the closed form, which tests/test_rowop_census_cpu.py holds to the
     oracle); a scale of 0 demands an error of 0.  With filter_neg the raw scores keep KINK of their magnitude from 0 in fp64;
  4. census: on integer data every output equals the fp64 value bit for bit, the sign of a zero included;
  5. untouched memory: every output NaN-filled inside sentinel bands before the call; no NaN left after it, every band around inputs and outputs
     intact (the band starts at row B: rows >= B of nothing are written), the inputs unchanged;
  6. attention backward with dmat only and with dsum only (torch.autograd.grad on one output; NULL for the other in the C call).
The worst margin of every row is printed; the module's margin_report fixture prints the worst per op and output after the last test."""
import ctypes

import numpy as np
import pytest
import torch

import _rowop_census as C
import _rowop_routes as T
from _guard import Buf

pytestmark = pytest.mark.gpu
USED = {}


@pytest.fixture(scope='module', autouse=True)
def margin_report():
    """after the last test of this module: the largest fraction of its bound that any row which ran used, per op and output"""
    yield
    for key in sorted({k for m in USED.values() for k in m}):
        sel = {n: m[key] for n, m in USED.items() if key in m}
        worst = max(sel, key=sel.get)
        print('%s.%s: at most %.4f of the bound (%s)' % (key + (sel[worst], worst)))


def P(q):
    return ctypes.c_void_p(q.ptr) if q is not None else None


def _ptrs(dev, bufs):
    return torch.tensor([b.ptr for b in bufs], dtype=torch.int64, device=dev)


def _settle(r, bufs, ins, outs):
    """after the calls: bands intact, no NaN left in an output, inputs unchanged"""
    torch.cuda.synchronize()
    for k, q in bufs.items():
        for i, b in enumerate(q if isinstance(q, list) else [q]):
            assert b is None or b.damaged() == 0, '%s: %d guard words of %s[%d] changed' % (r['name'], b.damaged(), k, i)
    for k, v in outs.items():
        assert not np.isnan(v).any(), '%s: %d NaN left in %s' % (r['name'], int(np.isnan(v).sum()), k)
    for k, (q, v) in ins.items():
        assert C.same_bits(q.get(v.shape), v), '%s: the input %s was written' % (r['name'], k)
    return outs


def run_c(dev, r, d):
    """the C entry points of row r on guard-banded buffers, after asking the route query about these very pointers"""
    from rec_now_amd import _lib
    lib = _lib.load()
    B, F, D, ld = r['B'], r['F'], r['D'], r['lead']
    bwd = C.has_bwd(r)
    st = _lib.stream()
    off = lambda q: int(q is not None and q.ptr % 16 != 0)                  # noqa: E731
    if r['op'] in ('fm', 'ipnn'):
        xs = [Buf(dev, B * D, d['x'][f]) for f in range(F)]
        dxs = [Buf(dev, B * D, lead=ld.get('dx', 0)) for _ in range(F)] if bwd else []
        xp, dxp = _ptrs(dev, xs), _ptrs(dev, dxs)
        assert all(q.ptr % 16 == 0 for q in xs) and all(q.ptr % 16 == 4 * ld.get('dx', 0) for q in dxs)
        ins = {'x[%d]' % f: (xs[f], d['x'][f]) for f in range(F)}
    if r['op'] == 'fm':
        y, S, g = Buf(dev, B), (Buf(dev, B * D) if r['has_S'] else None), Buf(dev, B, d['g'])
        assert lib.recnow_fm_route(0, B, F, D, int(S is not None)) == r['fwd'], 'forward route'
        _lib.call('recnow_fm_fwd', _lib.ptr(xp), F, B, D, P(y), P(S), st)
        outs = dict(y=y.get((B,)))
        if S is not None:
            outs['S'] = S.get((B, D))
        if bwd:
            assert lib.recnow_fm_route(1, B, F, D, 1) == r['bwd'], 'backward route'
            _lib.call('recnow_fm_bwd', _lib.ptr(xp), _lib.ptr(dxp), F, B, D, P(S), P(g), st)
            torch.cuda.synchronize()
            outs['dx'] = np.stack([q.get((B, D)) for q in dxs])
        ins['g'] = (g, d['g'])
        return _settle(r, dict(x=xs, dx=dxs, y=y, S=S, g=g), ins, outs)
    if r['op'] == 'ipnn':
        Pn = F * (F - 1) // 2
        out = Buf(dev, B * Pn, lead=ld.get('out', 0))
        dout = Buf(dev, B * Pn, d['dout'], lead=ld.get('dout', 0)) if bwd else None
        assert (off(out), off(dout) if bwd else T.masks(r)[1]) == T.masks(r)
        assert lib.recnow_inner_pnn_route(0, B, F, D, off(out)) == r['fwd'], 'forward route'
        assert lib.recnow_inner_pnn_route(1, B, F, D, off(dout)) == r['bwd'], 'backward route'
        _lib.call('recnow_inner_pnn_fwd', _lib.ptr(xp), F, B, D, P(out), st)
        outs = dict(out=out.get((B, Pn)))
        if bwd:
            _lib.call('recnow_inner_pnn_bwd', _lib.ptr(xp), _lib.ptr(dxp), F, B, D, P(dout), st)
            torch.cuda.synchronize()
            outs['dx'] = np.stack([q.get((B, D)) for q in dxs])
            ins['dout'] = (dout, d['dout'])
        return _settle(r, dict(x=xs, dx=dxs, out=out, dout=dout), ins, outs)
    L = F
    mk = lambda k, n, data=None: Buf(dev, n, data, lead=ld.get(k, 0))       # noqa: E731
    u, doc = mk('user', B * L * D, d['u']), mk('doc', B * D, d['doc'])
    mat, ssum = mk('mat', B * D), Buf(dev, B)
    dmat = mk('dmat', B * D, d['dmat']) if 'dmat' in d else None
    dsum = Buf(dev, B, d['dsum']) if 'dsum' in d else None
    du, dd = mk('duser', B * L * D), mk('ddoc', B * D)
    mf = off(u) * 1 | off(doc) * 2 | off(mat) * 4
    mb = off(u) * 1 | off(doc) * 2 | off(dmat) * 4 | off(du) * 8 | off(dd) * 16
    assert (mf, mb) == T.masks(r)
    assert lib.recnow_attention_dot_route(0, B, L, D, mf) == r['fwd'], 'forward route'
    assert lib.recnow_attention_dot_route(1, B, L, D, mb) == r['bwd'], 'backward route'
    fn = int(r['filter_neg'])
    _lib.call('recnow_attention_dot_fwd', P(u), P(doc), B, L, D, fn, P(mat), P(ssum), st)
    _lib.call('recnow_attention_dot_bwd', P(u), P(doc), P(dmat), P(dsum), B, L, D, fn, P(du), P(dd), st)
    torch.cuda.synchronize()
    outs = dict(mat=mat.get((B, D)), ssum=ssum.get((B,)), du=du.get((B, L, D)), ddoc=dd.get((B, D)))
    ins = dict(u=(u, d['u']), doc=(doc, d['doc']))
    ins.update({k: (q, d[k]) for k, q in (('dmat', dmat), ('dsum', dsum)) if q is not None})
    return _settle(r, dict(u=u, doc=doc, mat=mat, ssum=ssum, dmat=dmat, dsum=dsum, du=du, ddoc=dd), ins, outs)


def _dev_tensor(dev, a, view):
    """a on the device as a leaf that wants a gradient; view: a contiguous view that starts one float into a larger buffer"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not view:
        return t.to(dev).requires_grad_(True)
    buf = torch.zeros(t.numel() + 8, dtype=torch.float32, device=dev)
    buf[1:1 + t.numel()] = t.reshape(-1).to(dev)
    v = buf[1:1 + t.numel()].view(t.shape).detach().requires_grad_(True)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def has_public(r):
    """rows the layers can reach: they always pass S and allocate out / take dout on 16-byte boundaries"""
    return not (r['op'] == 'fm' and not r['has_S']) and not (r['op'] == 'ipnn' and r['lead'])


def run_public(dev, r, d):
    """forward and backward of row r through the public entry point"""
    from rec_now_amd import _lib
    from rec_now_amd.layers.fm_layer import FMLayer
    from rec_now_amd.layers.inner_pnn_layer import InnerPNNLayer
    from rec_now_amd.rec_block.attention import attention_by_dot_product
    lib = _lib.load()
    B, F, D = r['B'], r['F'], r['D']
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    if r['op'] in ('fm', 'ipnn'):
        xs = [_dev_tensor(dev, d['x'][f], r['view'] and f == 1) for f in range(F)]
        if r['op'] == 'fm':
            y = FMLayer()(xs)
            y.backward(up(d['g'])[:, None])
            return dict(y=y.detach().cpu().numpy()[:, 0], dx=np.stack([v.grad.cpu().numpy() for v in xs]))
        out = InnerPNNLayer()(xs)
        assert out.data_ptr() % 16 == 0 and lib.recnow_inner_pnn_route(0, B, F, D, 0) == r['fwd']
        res = dict(out=out.detach().cpu().numpy())
        if C.has_bwd(r):
            out.backward(up(d['dout']))
            res['dx'] = np.stack([v.grad.cpu().numpy() for v in xs])
        else:
            with pytest.raises(RuntimeError, match='RECNOW_EUNSUPPORTED'):          # a missing kernel is an error, never a fall-back
                out.backward(up(d['dout']) if 'dout' in d else torch.ones_like(out))
        return res
    u, doc = _dev_tensor(dev, d['u'], r['view']), _dev_tensor(dev, d['doc'], False)
    mask = T.ATTN_MIS['user'] * int(u.data_ptr() % 16 != 0)
    assert mask == T.masks(r)[0] and lib.recnow_attention_dot_route(0, B, F, D, mask) == r['fwd']
    mat, ssum = attention_by_dot_product(u, doc, r['filter_neg'])
    outs, ups = [], []
    if 'dmat' in d:
        outs.append(mat)
        ups.append(up(d['dmat']))
    if 'dsum' in d:
        outs.append(ssum)
        ups.append(up(d['dsum'])[:, None])
    du, dd = torch.autograd.grad(outs, [u, doc], ups)
    return dict(mat=mat.detach().cpu().numpy(), ssum=ssum.detach().cpu().numpy()[:, 0], du=du.cpu().numpy(), ddoc=dd.cpu().numpy())


def _bits(r, tag, got, want):
    for k, v in got.items():
        a, e = np.ascontiguousarray(v, np.float32).reshape(-1), want[k].astype(np.float32).reshape(-1)
        assert a.shape == e.shape
        bad = np.flatnonzero(a.view(np.int32) != e.view(np.int32))
        assert bad.size == 0, '%s census (%s): %d of %d words of %s differ from the exact value, first flat %d: %r vs %r' % (
            r['name'], tag, bad.size, a.size, k, bad[0], a[bad[0]], e[bad[0]])


@pytest.mark.parametrize('r', T.ROUTES, ids=[r['name'] for r in T.ROUTES])
def test_rowop_route(dev, r):
    public = has_public(r)
    # random data against fp64, entry by entry
    d = C.random_data(r)
    sc = C.compute(r, d, scales=True)
    ref = C.oracle(r, d)
    if r['op'] == 'attn' and r['filter_neg']:
        lo = float((np.abs(sc['sraw']) / sc['s_sraw']).min()) if sc['sraw'].size else np.inf
        assert lo >= C.KINK, 'a raw score %.3g of its magnitude from the clamp' % lo
    runs = ([('layer', run_public)] if public else []) + [('C', run_c)]
    worst = {}
    for tag, fn in runs:
        got = fn(dev, r, d)
        assert set(got) == set(C.outputs(r)) - ({'S'} if tag == 'layer' else set()), (tag, sorted(got))
        m = C.margins(r, got, ref, sc)
        print('%s (%s): fraction of the bound used %s' % (r['name'], tag, '  '.join('%s %.4f' % kv for kv in sorted(m.items()))))
        for k, v in m.items():
            worst[(r['op'], k)] = max(worst.get((r['op'], k), 0.0), v)
            assert v <= 1.0, '%s (%s): %s is %.3g times the bound (1e-5 of the entry\'s cancellation-free scale)' % (r['name'], tag, k, v)
    USED[r['name']] = worst
    # census data, bit for bit (tests/test_rowop_census_cpu.py: every row keeps the first ladder entry)
    c, _ = C.make(r, params=C.LADDER[0])
    want = C.exact(r, c)
    _bits(r, 'C', run_c(dev, r, c), want)
    if public:
        _bits(r, 'layer', run_public(dev, r, c), want)
