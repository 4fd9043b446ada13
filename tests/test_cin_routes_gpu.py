"""Every path through recnow_cin_fwd / recnow_cin_bwd (tests/_cin_routes.py), bit for bit on integer census data (tests/_cin_census.py), inside
guard bands, through the C ABI.  Each row, in each of its (output_input, sum_channel) modes, checks:
  1. census bits: out, demb and every dW_k equal the exact census element for element; after the forward the saved buffer's x0t and X_k do too;
  2. guard bands: out, demb and every dW_k sit in sentinel-filled buffers with 256 words on each side: every sentinel outside the logical array
     survives and every word inside has been written; `saved` and `ws` carry a sentinel tail past recnow_cin_saved_bytes /
     recnow_cin_workspace_bytes that survives; `ws` is filled with NaN before the forward and again before the backward, so a product that
     accumulates into an unseeded buffer cannot pass;
  3. route taken: the forward launches exactly L hooked products with the row's tile-family tags, the backward sum_k (1 if fused else 3): the
     fused kernel (no profiler hook) ran where the table says so and nowhere else;
  4. a planted NaN in one sample's embedding makes exactly the elements of out and demb non-finite that the fp64 restatement makes non-finite
     -- all of them inside that sample -- and every other element is bit-identical to the clean run;
  5. random data (x ~ N(0, 0.5), W ~ U(-0.5, 0.5)): per element |got - ref|_i <= C_i maj_i against oracle/dense_ref.cin_layer in fp64 autograd,
     maj the same computation on |x|, |W|, |dout|, C_i the sum of the per-product constants on the longest path into the output;
  6. reproducibility: a second backward on the random data returns every output bit for bit.
test_misaligned_* : every W_k a contiguous view one float into a larger buffer, at a shape whose sizes the fused kernel takes."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import _cin_census as C
import _cin_routes as T
import dense_ref as R
from _cin_routes import ROUTES, MISALIGNED, spec
from test_gemm_routes_gpu import C_ELEM, SENT

pytestmark = pytest.mark.gpu

C_FUSED = C.C_FUSED               # per-product constant of k_cin_bwd_fused: 2.4 x the 1.6e-7 a host fp32 emulation of its summation orders gave
PAD = 256                         # guard words before and after every output
TAIL = 4096                       # sentinel words past the saved buffer and the workspace
USED = {}                         # row / mode / output -> largest fraction of the random-data bound used


def _sent():
    return float(np.array([SENT], np.uint32).view(np.float32)[0])


class Guard:
    """n floats inside a sentinel-filled flat buffer, PAD words on each side, the first `off` floats past a 1 KiB boundary"""

    def __init__(self, dev, n, off=0, data=None):
        self.n, self.lo = n, PAD + off
        self.buf = torch.full((PAD + off + n + PAD,), _sent(), dtype=torch.float32, device=dev)
        if data is not None:
            self.buf[self.lo:self.lo + n].copy_(torch.from_numpy(np.ascontiguousarray(data, np.float32).reshape(-1)).to(dev))
        self.ptr = self.buf.data_ptr() + 4 * self.lo

    def check(self, what, written=True):
        bits = self.buf.view(torch.int32).cpu().numpy()
        inside = bits[self.lo:self.lo + self.n]
        outside = np.concatenate([bits[:self.lo], bits[self.lo + self.n:]])
        assert (outside == SENT).all(), '%s: %d guard words changed' % (what, int((outside != SENT).sum()))
        if written:
            assert (inside != SENT).all(), '%s: %d words inside were never written' % (what, int((inside == SENT).sum()))
        return inside.view(np.float32).copy()


def _tags(lib, cap=64):
    t, t0, t1 = (ctypes.c_int * cap)(), (ctypes.c_double * cap)(), (ctypes.c_double * cap)()
    n = lib.recnow_prof_intervals(t, t0, t1, cap)
    assert n >= 0
    return [t[i] for i in range(n)]


def run(dev, s, oi, sc, emb, Ws, dout, w_off=0, prof=False, twice=False):
    """recnow_cin_fwd, then recnow_cin_bwd (twice: a second time into fresh buffers) on one stack; checks every guard band.  Returns a dict with
    out, demb, dW[l], x0t, X[l] (numpy), fwd_tags / bwd_tags (with prof) and second (demb, dW of the second backward)."""
    from rec_now_amd import _lib
    lib = _lib.load()
    B, D, F, Hs = s['B'], s['D'], s['F'], list(s['Hs'])
    M, L, ext = B * D, len(Hs), [F] + list(Hs)
    ctot = (F if oi else 0) + sum(Hs)
    hid = (ctypes.c_int * L)(*Hs)
    sb, wb = int(lib.recnow_cin_saved_bytes(B, D, F, hid, L)), int(lib.recnow_cin_workspace_bytes(B, D, F, hid, L))
    assert sb % 4 == 0 and wb % 4 == 0
    embd = torch.from_numpy(np.ascontiguousarray(emb, np.float32)).to(dev)
    doutd = torch.from_numpy(np.ascontiguousarray(dout, np.float32)).to(dev)
    Wg = [Guard(dev, w.size, off=w_off, data=w) for w in Ws]
    wptr = (ctypes.c_void_p * L)(*[g.ptr for g in Wg])
    out = Guard(dev, B * (D if sc else ctot * D))
    saved = torch.full((sb // 4 + TAIL,), _sent(), dtype=torch.float32, device=dev)
    ws = torch.full((wb // 4 + TAIL,), float('nan'), dtype=torch.float32, device=dev)
    ws[wb // 4:] = _sent()
    res = {}

    def tails(when):
        assert bool((saved[sb // 4:].view(torch.int32) == SENT).all()), '%s: saved written past recnow_cin_saved_bytes = %d' % (when, sb)
        assert bool((ws[wb // 4:].view(torch.int32) == SENT).all()), '%s: workspace written past recnow_cin_workspace_bytes = %d' % (when, wb)

    if prof:
        _lib.check(lib.recnow_prof_enable(64), 'recnow_prof_enable')
        _lib.check(lib.recnow_prof_sample_every(1), 'recnow_prof_sample_every')
    try:
        _lib.call('recnow_cin_fwd', _lib.ptr(embd), wptr, B, D, F, hid, L, oi, sc, ctypes.c_void_p(out.ptr), _lib.ptr(saved), sb, _lib.ptr(ws), wb,
                  _lib.stream())
        torch.cuda.synchronize()
        if prof:
            res['fwd_tags'] = _tags(lib)
        tails('forward')
        res['out'] = out.check('out').reshape(B, -1)
        sv = saved[:sb // 4].cpu().numpy()
        off = 0
        res['x0t'] = sv[:M * F].reshape(M, F).copy()
        off += (M * F * 4 + 255) // 256 * 64
        res['X'] = []
        for h in Hs:
            res['X'].append(sv[off:off + M * h].reshape(M, h).copy())
            off += (M * h * 4 + 255) // 256 * 64
        for rep in range(2 if twice else 1):
            ws[:wb // 4] = float('nan')
            demb = Guard(dev, B * F * D)
            dW = [Guard(dev, w.size) for w in Ws]
            dptr = (ctypes.c_void_p * L)(*[g.ptr for g in dW])
            _lib.call('recnow_cin_bwd', wptr, _lib.ptr(doutd), _lib.ptr(saved), sb, B, D, F, hid, L, oi, sc, ctypes.c_void_p(demb.ptr), dptr,
                      _lib.ptr(ws), wb, _lib.stream())
            torch.cuda.synchronize()
            if prof and rep == 0:
                res['bwd_tags'] = _tags(lib)
            tails('backward')
            got = (demb.check('demb').reshape(B, F * D), [g.check('dW%d' % l).reshape(Ws[l].shape) for l, g in enumerate(dW)])
            if rep == 0:
                res['demb'], res['dW'] = got
            else:
                res['second'] = got
        for l, g in enumerate(Wg):
            g.check('W%d (an input)' % l)
        assert torch.equal(embd.cpu(), torch.from_numpy(np.ascontiguousarray(emb, np.float32))) or np.isnan(emb).any()
    finally:
        if prof:
            lib.recnow_prof_enable(0)
    return res


def _same(tag, got, want):
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want).astype(np.float32).reshape(-1)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    wrong = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
    assert wrong.size == 0, '%s: %d of %d differ from the census, first flat %d: %r vs %r' % (tag, wrong.size, want.size, wrong[0], got[wrong[0]],
                                                                                          want[wrong[0]])


def _constants(fused):
    """sum of the per-product constants on the longest path into out, demb and dW_l (layers 0-based).  X_l carries l forward products; the data
    gradient that reaches layer l has passed the backward products of the layers above; dx0 collects one product per layer (the L adds into it
    count as one more product), dW_l is one product of dX_{l+1} and X_l.  k_rowsum's channel sums count as one product."""
    L = len(fused)
    cb = [C_FUSED if f else C_ELEM for f in fused]
    above = [sum(cb[l + 1:]) for l in range(L)]                     # into dX_{l+1}
    c_out = (L + 1) * C_ELEM
    c_demb = max(l * C_ELEM + above[l] + cb[l] for l in range(L)) + C_ELEM
    c_dw = [l * C_ELEM + above[l] + C_ELEM for l in range(L)]
    return c_out, c_demb, c_dw


def _reference(c, r, oi, sc, emb, Ws, dout):
    """out, demb, dW_l in fp64: oracle/dense_ref.cin_layer under autograd; beyond 2048 rows (the (B, D, F, H) tensor of the line-by-line form
    does not fit a test) the fp64 restatement, which tests/test_cin_census_cpu.py holds to cin_layer at the small shapes"""
    if r['B'] * r['D'] > C.DENSE_ROWS:
        ref = C.restate(c, oi, sc, inp=(emb, Ws, dout))
        return ref['out'], ref['demb'], [ref['dW%d' % l] for l in range(len(Ws))]
    x = torch.from_numpy(emb).double().requires_grad_(True)
    ws = [torch.from_numpy(w).double().reshape(1, 1, *w.shape).requires_grad_(True) for w in Ws]
    y = R.cin_layer(x, ws, r['F'], r['D'], bool(oi), bool(sc))
    y.backward(torch.from_numpy(dout).double())
    return y.detach().numpy(), x.grad.numpy(), [w.grad.numpy().reshape(Ws[l].shape) for l, w in enumerate(ws)]


def check_row(dev, r, w_off=0):
    from rec_now_amd import _lib
    _lib.call('recnow_set_gemm_precision', 0)
    s = spec(r)
    B, D, F, Hs = r['B'], r['D'], r['F'], list(r['Hs'])
    L = len(Hs)
    c = C.make(modes=r['modes'], params=r['census'], verify=False, **s)            # (the CPU census test has verified these parameters)
    fused = r['fused']
    for oi, sc in r['modes']:
        tag = '%s mode %d%d' % (r['name'], oi, sc)
        want = C.expected(c, oi, sc)
        dout = c.dout(oi, sc)
        # 1-3: census bits, guard bands, route
        got = run(dev, s, oi, sc, c.emb, c.W, dout, w_off=w_off, prof=True)
        assert tuple(got['fwd_tags']) == r['tags'], '%s: forward launches %r, the table says %r' % (tag, got['fwd_tags'], r['tags'])
        assert len(got['bwd_tags']) == T.bwd_launches(fused), '%s: %d hooked backward products %r, the table says %d (fused %r)' % (
            tag, len(got['bwd_tags']), got['bwd_tags'], T.bwd_launches(fused), fused)
        _same(tag + ' out', got['out'], want['out'])
        _same(tag + ' saved x0t', got['x0t'], want['x0t'])
        for l in range(L):
            _same(tag + ' saved X%d' % (l + 1), got['X'][l], want['X%d' % (l + 1)])
        _same(tag + ' demb', got['demb'], want['demb'])
        for l in range(L):
            _same(tag + ' dW%d' % l, got['dW'][l], want['dW%d' % l])
        # 4: a NaN in one sample's embedding
        rng = np.random.default_rng(zlib.crc32(tag.encode()))
        b0 = int(rng.integers(B))
        embn = c.emb.copy()
        embn[b0, int(rng.integers(F * D))] = np.nan
        with np.errstate(invalid='ignore'):
            ref = C.restate(c, oi, sc, inp=(embn, c.W, dout))
        bad = run(dev, s, oi, sc, embn, c.W, dout, w_off=w_off)
        for k in ('out', 'demb'):
            nf = ~np.isfinite(ref[k])
            assert nf[b0].any() and not np.delete(nf, b0, 0).any()
            assert not np.isfinite(bad[k][nf]).any(), '%s NaN: %d elements of %s with a non-finite reference are finite' % (
                tag, int(np.isfinite(bad[k][nf]).sum()), k)
            assert np.array_equal(bad[k][~nf].view(np.int32), got[k][~nf].view(np.int32)), '%s NaN: %d finite elements of %s moved' % (
                tag, int((bad[k][~nf] != got[k][~nf]).sum()), k)
        # 5, 6: random data per element against fp64; the backward twice
        emb = rng.normal(0, 0.5, c.emb.shape).astype(np.float32)
        Ws = [rng.uniform(-0.5, 0.5, w.shape).astype(np.float32) for w in c.W]
        dr = (rng.normal(0, 1, dout.shape) * (dout != 0)).astype(np.float32)            # (beyond 2048 rows: on the census's rows)
        rnd = run(dev, s, oi, sc, emb, Ws, dr, w_off=w_off, twice=True)
        assert np.array_equal(rnd['demb'].view(np.int32), rnd['second'][0].view(np.int32)), tag + ': demb differs between two backward calls'
        for l in range(L):
            assert np.array_equal(rnd['dW'][l].view(np.int32), rnd['second'][1][l].view(np.int32)), tag + ': dW%d differs between two calls' % l
        ro, rd, rw = _reference(c, r, oi, sc, emb, Ws, dr)
        maj = C.majorant(c, oi, sc, inp=(emb, Ws, dr), fused=fused)
        c_out, c_demb, c_dw = _constants(fused)
        items = [('out', rnd['out'], ro, c_out * maj['out']), ('demb', rnd['demb'], rd, c_demb * maj['demb'])]
        items += [('dW%d' % l, rnd['dW'][l], rw[l], c_dw[l] * maj['dW%d' % l]) for l in range(L)]
        for k, g, ref_, lim in items:
            assert np.isfinite(g).all(), '%s random: non-finite %s' % (tag, k)
            err = np.abs(g.astype(np.float64) - ref_)
            frac = float((err[lim > 0] / lim[lim > 0]).max()) if (lim > 0).any() else 0.0
            USED[(r['name'], oi, sc, k)] = frac
            print('%s random %s: largest fraction of the bound used %.3f' % (tag, k, frac))
            assert (err <= lim).all(), '%s random: %d elements of %s beyond the per-element bound, worst fraction %.3g' % (
                tag, int((err > lim).sum()), k, frac)


@pytest.mark.parametrize('r', ROUTES, ids=[r['name'] for r in ROUTES])
def test_cin_route(dev, r):
    check_row(dev, r)


def test_bound_use_report(dev):
    """the largest fraction of its random-data bound any row used (printed; the rows assert the bound)"""
    if not USED:
        return
    for k in ('out', 'demb', 'dW'):
        sel = {key: v for key, v in USED.items() if key[3].startswith(k)}
        worst = max(sel, key=sel.get)
        print('%s: at most %.3f of the bound (%s mode %d%d %s)' % ((k, sel[worst]) + worst))
    assert max(USED.values()) <= 1.0


def test_misaligned_weights_c_abi(dev):
    """every W_k one float past a 16-byte boundary, sizes that fit k_cin_bwd_fused<128>: the forward takes the edge kernels, the backward the
    two products (3 hooked launches per layer) -- not RECNOW_EUNSUPPORTED -- and both match the census"""
    check_row(dev, MISALIGNED, w_off=1)


def test_misaligned_weights_layer(dev):
    """the same through CINLayer: each weight a contiguous view one float into a larger buffer (_lib.f32c does not realign it)"""
    from rec_now_amd.layers.cin_layer import CINLayer
    r = MISALIGNED
    c = C.make(modes=r['modes'], params=r['census'], verify=False, **spec(r))
    for oi, sc in r['modes']:
        want = C.expected(c, oi, sc)
        layer = CINLayer(list(r['Hs']), embedding_dim=r['D'])
        x = torch.from_numpy(c.emb).to(dev).requires_grad_(True)
        layer(x, bool(oi), bool(sc))
        for l, w in enumerate(c.W):
            buf = torch.zeros(w.size + 5, device=dev)
            view = buf[1:1 + w.size].view(1, 1, *w.shape)
            view.copy_(torch.from_numpy(w).to(dev))
            assert view.is_contiguous() and view.data_ptr() % 16 == 4
            layer.idx2weight[l + 1] = view.requires_grad_(True)
        y = layer(x, bool(oi), bool(sc))
        y.backward(torch.from_numpy(c.dout(oi, sc)).to(dev))
        _same('layer out', y.detach().cpu().numpy(), want['out'])
        _same('layer demb', x.grad.cpu().numpy(), want['demb'])
        for l in range(len(c.W)):
            _same('layer dW%d' % l, layer.idx2weight[l + 1].grad.cpu().numpy(), want['dW%d' % l])


def test_empty_batch(dev):
    """B = 0 with NULL tensor pointers and 0-byte buffers: both calls succeed, the sentinel-filled dW buffers come back all zero, guards intact"""
    from rec_now_amd import _lib
    lib = _lib.load()
    D, F, Hs = 16, 4, (64, 32)
    ext = [F] + list(Hs)
    hid = (ctypes.c_int * 2)(*Hs)
    wptr = (ctypes.c_void_p * 2)(None, None)
    assert int(lib.recnow_cin_saved_bytes(0, D, F, hid, 2)) >= 0
    for oi, sc in T.ALL4:
        _lib.call('recnow_cin_fwd', None, wptr, 0, D, F, hid, 2, oi, sc, None, None, 0, None, 0, _lib.stream())
        dW = [Guard(dev, ext[l + 1] * F * ext[l]) for l in range(2)]
        dptr = (ctypes.c_void_p * 2)(*[g.ptr for g in dW])
        _lib.call('recnow_cin_bwd', wptr, None, None, 0, 0, D, F, hid, 2, oi, sc, None, dptr, None, 0, _lib.stream())
        torch.cuda.synchronize()
        for l, g in enumerate(dW):
            v = g.check('dW%d at B = 0' % l)
            assert not v.view(np.int32).any(), 'dW%d at B = 0 is not all zero' % l
