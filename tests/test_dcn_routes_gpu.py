"""Every path through recnow_dcn_fwd / recnow_dcn_bwd and the step route (tests/_dcn_routes.py), through the C ABI on guard-banded buffers
(tests/_guard.py).  Each row checks:
  1. route: recnow_dcn_route answers the row's codes for the very pointers the call is made with;
  2. guard bands: every output NaN-filled before the call, no NaN left after it, every sentinel around inputs, outputs and the workspace intact;
  3. fp64: y and dx per row, csave per entry, dkernels and dbiases per layer and column against oracle/dense_ref.dcn_layer under fp64 autograd, at
     1e-5 of the cancellation-free magnitude of what was summed (tests/_dcn_census.py margins(): NOT the maximum of the tensor).  The data keeps
     c_l and dc_l off 0 (random_data()); tests/test_dcn_census_cpu.py holds an fp32 restatement of the kernels to half this bound on every row;
  4. reproducibility: a second forward and backward return every output bit for bit (fixed summation order, no float atomics);
  5. linear (and relu) rows: on integer census data the GPU result equals the fp64 value to the bit (zero signs included, except dx of the general
     backward, see there).
The worst margin of every row is printed; the module's margin_report fixture prints the worst per output after the last test."""
import ctypes

import numpy as np
import pytest
import torch

import _dcn_census as C
import _dcn_routes as T
import dense_ref as R
from _guard import Buf

pytestmark = pytest.mark.gpu
USED = {}


@pytest.fixture(scope='module', autouse=True)
def margin_report():
    """after the last test of this module: the largest fraction of its bound that any row which ran used, per output (the rows assert the bound)"""
    yield
    for k in sorted({k for m in USED.values() for k in m}):
        sel = {n: m[k] for n, m in USED.items() if k in m}
        worst = max(sel, key=sel.get)
        print('%s: at most %.4f of the bound (%s)' % (k, sel[worst], worst))


def _oracle(r, x, w, b, dy):
    """y, dx, dW, db of oracle/dense_ref.dcn_layer in fp64 autograd, c_l from its own lines in torch fp64; the scales from the closed form, which must
    agree with autograd"""
    L = r['L']
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    ks = [torch.from_numpy(w[l][:, None]).double().requires_grad_(True) for l in range(L)]
    bs = [torch.from_numpy(b[l][None]).double().requires_grad_(True) for l in range(L)] if b is not None else None
    y = R.dcn_layer(x64, ks, bs, C.ACT_ORACLE[r['act']])
    y.backward(torch.from_numpy(dy).double())
    ref = dict(y=y.detach().numpy(), dx=x64.grad.numpy(), dW=np.stack([k.grad.numpy()[:, 0] for k in ks]),
               db=np.stack([v.grad.numpy()[0] for v in bs]) if bs is not None else None)
    sc = C.cross(x, w, b, dy, r['act'], scales=True)
    for k in ('y', 'dx', 'dW') + (('db',) if bs is not None else ()):
        assert np.abs(sc[k] - ref[k]).max() <= 1e-11 * max(1.0, np.abs(ref[k]).max()), 'the closed form and the autograd oracle disagree on ' + k
    # dense_ref.dcn_layer does not return the scalars c_l = x_l @ kernel_l: the same lines again in torch fp64, layer by layer
    with torch.no_grad():
        act, xl, cs = R._act(C.ACT_ORACLE[r['act']]), x64, []
        for l in range(L):
            cs.append(xl @ ks[l])
            xl = act(x64 * cs[-1] + (bs[l] if bs is not None else 0))
        assert torch.equal(xl, y.detach())
    ref['c'] = torch.cat(cs, 1).numpy()
    return ref, sc


def run(dev, r, x, w, b, dy):
    """recnow_dcn_fwd then recnow_dcn_bwd on guard-banded buffers; returns y, c (None without csave), dx, dW, db (None without bias)"""
    from rec_now_amd import _lib
    lib = _lib.load()
    B, D, L, ld = r['B'], r['D'], r['L'], r['lead']
    xb = Buf(dev, B * D, x, lead=ld.get('x', 0))
    kb = Buf(dev, L * D, w, lead=ld.get('kernels', 0))
    bb = Buf(dev, L * D, b, lead=ld.get('biases', 0)) if b is not None else None
    gb = Buf(dev, B * D, dy, lead=ld.get('dy', 0))
    yb, dxb = Buf(dev, B * D, lead=ld.get('y', 0)), Buf(dev, B * D, lead=ld.get('dx', 0))
    cb = Buf(dev, B * L) if r['csave'] else None
    dkb = Buf(dev, L * D)
    dbb = Buf(dev, L * D) if b is not None else None
    wbytes = int(lib.recnow_dcn_workspace_bytes(B, D, L))
    assert wbytes % 4 == 0
    ws = Buf(dev, wbytes // 4)
    P = lambda q: ctypes.c_void_p(q.ptr) if q is not None else None          # noqa: E731
    mis = lambda q: 1 if (q is not None and q.ptr % 16) else 0                  # noqa: E731
    mf = mis(xb) * T.MIS_X | mis(yb) * T.MIS_Y | mis(kb) * T.MIS_K | mis(bb) * T.MIS_B
    mb = mis(xb) * T.MIS_X | mis(gb) * T.MIS_Y | mis(dxb) * T.MIS_DX | mis(kb) * T.MIS_K | mis(bb) * T.MIS_B
    assert (mf, mb) == T.masks(r)
    assert lib.recnow_dcn_route(0, B, D, L, int(r['csave']), mf) == r['fwd'], 'forward route'
    assert lib.recnow_dcn_route(1, B, D, L, int(r['csave']), mb) == r['bwd'], 'backward route'
    _lib.call('recnow_dcn_fwd', P(xb), P(kb), P(bb), B, D, L, r['act'], P(yb), P(cb), _lib.stream())
    _lib.call('recnow_dcn_bwd', P(xb), P(kb), P(bb), P(gb), P(cb), B, D, L, r['act'], P(dxb), P(dkb), P(dbb), P(ws), wbytes, _lib.stream())
    torch.cuda.synchronize()
    bufs = dict(x=xb, kernels=kb, biases=bb, dy=gb, y=yb, dx=dxb, csave=cb, dkernels=dkb, dbiases=dbb, workspace=ws)
    for k, q in bufs.items():
        if q is not None:
            assert q.damaged() == 0, '%s: %d guard words of %s changed' % (r['name'], q.damaged(), k)
    out = dict(y=yb.get((B, D)), c=cb.get((B, L)) if cb else None, dx=dxb.get((B, D)), dW=dkb.get((L, D)), db=dbb.get((L, D)) if dbb else None)
    for k, v in out.items():
        assert v is None or not np.isnan(v).any(), '%s: %d NaN left in %s' % (r['name'], int(np.isnan(v).sum()), k)
    for k, q, v in (('x', xb, x), ('kernels', kb, w), ('dy', gb, dy)):
        assert C.same_bits(q.get(v.shape), v), '%s: the input %s was written' % (r['name'], k)
    return out


def _bits_equal(tag, a, b):
    for k in a:
        if a[k] is not None:
            assert C.same_bits(a[k], b[k]), '%s: %s differs in %d words' % (tag, k, int((a[k].view(np.int32) != b[k].view(np.int32)).sum()))


@pytest.mark.parametrize('r', T.ROUTES, ids=[r['name'] for r in T.ROUTES])
def test_dcn_route(dev, r):
    x, w, b, dy = C.random_data(r)
    if r['act'] == C.RELU:
        lo = C.min_preact(x, w, b, r['act'])[0]
        assert lo >= C.KINK, 'a pre-activation %.3g from the kink' % lo
    ref, sc = _oracle(r, x, w, b, dy)
    got = run(dev, r, x, w, b, dy)
    _bits_equal(r['name'] + ' second run', got, run(dev, r, x, w, b, dy))
    m = C.margins(got, ref, sc)
    USED[r['name']] = m
    print('%s: fraction of the bound used %s' % (r['name'], '  '.join('%s %.4f' % kv for kv in sorted(m.items()))))
    assert set(m) == {'y', 'dx', 'dW'} | ({'c'} if r['csave'] else set()) | ({'db'} if r['bias'] else set())
    for k, v in m.items():
        assert v <= 1.0, '%s: %s is %.3g times the bound (1e-5 of the cancellation-free scale)' % (r['name'], k, v)
    if r['act'] in (C.LINEAR, C.RELU):
        c = C.make(r, r['act'], params=C.LADDER[0])                 # (tests/test_dcn_census_cpu.py: every row keeps the first ladder entry)
        want = C.exact(c)
        cen = run(dev, r, c.x, c.w, c.b, c.dy)
        for k, v in cen.items():
            if v is not None:
                # bit for bit, the sign of a zero included -- but for dx of the general backward: k_dcn_bwd_rows_general starts a row's dx from
                # dc_0 * w_0, which is -0 where dc_0 = 0 and w_0 < 0 (rows without gradient), and adds +-0 terms; the closed form starts from +0
                fold = np.float32(0) if (k == 'dx' and r['bwd'] // 100000 == T.B_GENERAL) else None
                a, e = v.reshape(-1), want[k].astype(np.float32).reshape(-1)
                if fold is not None:
                    a, e = a + fold, e + fold
                bad = np.flatnonzero(a.view(np.int32) != e.view(np.int32))
                assert bad.size == 0, '%s census: %d of %d words of %s differ from the exact value, first flat %d: %r vs %r' % (
                    r['name'], bad.size, v.size, k, bad[0], v.reshape(-1)[bad[0]], want[k].reshape(-1)[bad[0]])


def _step_data(s):
    import zlib
    rng = np.random.default_rng(zlib.crc32(('dcn step ' + s['name']).encode()))
    B, D = s['B'], s['D']
    off = lambda: rng.uniform(0.5, 1.5, (B, 1)) * rng.choice([-1.0, 1.0], (B, 1))      # noqa: E731
    x0, xl, dz = ((rng.normal(0, 1, (B, D)) + off()).astype(np.float32) for _ in range(3))
    w = ((rng.uniform(-1, 1, D) + 0.75) / D).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, D).astype(np.float32) if s['bias'] else None
    return x0, xl, w, b, dz


def _step_run(dev, s, x0, xl, w, b, dz):
    from rec_now_amd import _lib
    lib = _lib.load()
    B, D, act = s['B'], s['D'], s['act']
    # every tensor one float off a 16-byte boundary: the step route promises any alignment
    ins = {k: Buf(dev, v.size, v, lead=1) for k, v in (('x0', x0), ('xl', xl), ('w', w), ('dz', dz))}
    bb = Buf(dev, D, b, lead=1) if b is not None else None
    z, cb, dx0, dxl = Buf(dev, B * D, lead=1), Buf(dev, B, lead=1), Buf(dev, B * D, lead=1), Buf(dev, B * D, lead=1)
    dw, db = Buf(dev, D, lead=1), (Buf(dev, D, lead=1) if b is not None else None)
    wbytes = int(lib.recnow_dcn_step_workspace_bytes(B, D))
    ws = Buf(dev, wbytes // 4)
    P = lambda q: ctypes.c_void_p(q.ptr) if q is not None else None          # noqa: E731
    _lib.call('recnow_dcn_step_fwd', P(ins['x0']), P(ins['xl']), P(ins['w']), P(bb), B, D, act, P(z), P(cb), _lib.stream())
    _lib.call('recnow_dcn_step_bwd', P(ins['x0']), P(ins['xl']), P(ins['w']), P(z), P(cb), P(ins['dz']), B, D, act, P(dx0), P(dxl), P(dw), P(db), P(ws),
              wbytes, _lib.stream())
    torch.cuda.synchronize()
    for k, q in list(ins.items()) + [('b', bb), ('z', z), ('c', cb), ('dx0', dx0), ('dxl', dxl), ('dw', dw), ('db', db), ('workspace', ws)]:
        assert q is None or q.damaged() == 0, '%s: guard words of %s changed' % (s['name'], k)
    out = dict(z=z.get((B, D)), c=cb.get((B,)), dx0=dx0.get((B, D)), dxl=dxl.get((B, D)), dw=dw.get((D,)), db=db.get((D,)) if db else None)
    for k, v in out.items():
        assert v is None or not np.isnan(v).any(), '%s: NaN left in %s' % (s['name'], k)
    return out


@pytest.mark.parametrize('s', T.STEPS, ids=[s['name'] for s in T.STEPS])
def test_dcn_step_route(dev, s):
    """one cross layer with its own layer input: z = act(x0 (x_l . w) + b) against fp64 autograd.  Scales: c sum_d |x_l,d w_d|; z per row
    max |x0| sum |x_l w| + max |b|; dx0 = dz' c per row max |dz'| sum |x_l w|; dx_l = dc w per row sum_d |dz'_d x0_d| max |w|; dw per column
    sum_rows |x_l,d dc|, db sum_rows |dz'_d|  (dz' = dz act'(z))."""
    x0, xl, w, b, dz = _step_data(s)
    t = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in (('x0', x0), ('xl', xl), ('w', w))}
    tb = torch.from_numpy(b).double().requires_grad_(True) if b is not None else None
    c64 = t['xl'] @ t['w']
    pre = t['x0'] * c64[:, None] + (tb if tb is not None else 0)
    z64 = {C.LINEAR: lambda v: v, C.TANH: torch.tanh}[s['act']](pre)
    z64.backward(torch.from_numpy(dz).double())
    zz = z64.detach().numpy()
    dzp = dz.astype(np.float64) * C.act_grad_from_out(zz, s['act'])
    s_c = np.abs(xl.astype(np.float64) * w).sum(1)
    s_dc = np.abs(dzp * x0).sum(1)
    dc = (dzp * x0).sum(1)
    got = _step_run(dev, s, x0, xl, w, b, dz)
    _bits_equal(s['name'] + ' second run', got, _step_run(dev, s, x0, xl, w, b, dz))
    rel, tiny = C.REL, 1e-300
    rowm = lambda g, ref, sc: float((np.abs(g - ref).max(1) / np.maximum(rel * sc, tiny)).max())      # noqa: E731
    m = {'c': float((np.abs(got['c'] - c64.detach().numpy()) / np.maximum(rel * s_c, tiny)).max()),
         'z': rowm(got['z'], zz, np.abs(x0).max(1) * s_c + (np.abs(b).max() if b is not None else 0)),
         'dx0': rowm(got['dx0'], t['x0'].grad.numpy(), np.abs(dzp).max(1) * s_c),
         'dxl': rowm(got['dxl'], t['xl'].grad.numpy(), s_dc * np.abs(w).max()),
         'dw': float((np.abs(got['dw'] - t['w'].grad.numpy()) / np.maximum(rel * np.abs(xl * dc[:, None]).sum(0), tiny)).max())}
    if b is not None:
        m['db'] = float((np.abs(got['db'] - tb.grad.numpy()) / np.maximum(rel * np.abs(dzp).sum(0), tiny)).max())
    USED[s['name']] = m
    print('%s: fraction of the bound used %s' % (s['name'], '  '.join('%s %.4f' % kv for kv in sorted(m.items()))))
    for k, v in m.items():
        assert v <= 1.0, '%s: %s is %.3g times the bound' % (s['name'], k, v)
