"""Every MultiDense route (tests/_dense_routes.py) through the C ABI (recnow_multi_dense_fwd / _bwd, workspace of
recnow_multi_dense_workspace_bytes), per row of the table:
  1. guard bands: y, dx, dkernel, dbias and the workspace have a sentinel tail (and, for an offset pointer, a sentinel lead); the outputs are NaN
     before the call, the workspace is NaN before the forward and NaN again before the backward: every sentinel word survives, every declared
     output word is written;
  2. route proof: with recnow_prof_enable / recnow_prof_sample_every(1) the GEMM-family tags recorded by the forward call and by the backward call
     are as many as the table's gemm_fwd / gemm_bwd -- none exactly when no product of the call takes the GEMM;
  3. integer data (integers times powers of two), LINEAR and RELU: y, dx, dkernel, dbias equal the fp64 reference bit for bit (-0.0 taken as +0.0);
  4. random data (TANH / SIGMOID / LINEAR by turns; rows of x and columns of kernel scaled by 2^-k, k = 0..8): each row of y and dx within
     1e-5 x the row's max |ref|, each entry of dkernel and dbias within 1e-5 x the fp64 sum of |terms| of that entry, and the norm bound of the
     layer tests (_chunked_oracle.close); the worst margin of the row is printed as a fraction of its bound."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, 'oracle')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _dense_routes as T                      # noqa: E402
from _guard import Buf                         # noqa: E402

pytestmark = pytest.mark.gpu

REL = 1e-5                         # the project's bound (tests/test_mix_routes_gpu.py REL)
RANDOM_ACTS = (T.TANH, T.SIGMOID, T.LINEAR)


def _gemm_tags(lib):
    cap = 256
    t, t0, t1 = (ctypes.c_int * cap)(), (ctypes.c_double * cap)(), (ctypes.c_double * cap)()
    n = lib.recnow_prof_intervals(t, t0, t1, cap)
    assert 0 <= n < cap, n
    return [t[i] for i in range(n) if t[i] in T.GEMM_TAGS]


def run(dev, r, inp, act, prof=False):
    """forward and backward of row r.  Returns (outputs, (GEMM tags of the forward, of the backward) or None) and checks every sentinel."""
    import torch
    from rec_now_amd import _lib
    lib = _lib.load()
    B, D, U, N, xb = r['B'], r['D'], r['U'], r['N'], r['x_batched']
    x = Buf(dev, inp['x'].size, inp['x'], lead=r['x_off'])
    kernel, bias, dy = Buf(dev, N * D * U, inp['kernel']), Buf(dev, N * U, inp['bias']), Buf(dev, N * B * U, inp['dy'])
    wb = int(lib.recnow_multi_dense_workspace_bytes(B, D, U, N))
    ws = Buf(dev, wb // 4)
    assert wb % 4 == 0
    outs = {'y': Buf(dev, N * B * U)}
    shapes = {'y': (N, B, U), 'dx': (N, B, D) if xb else (B, D), 'dkernel': (N, D, U), 'dbias': (N, U)}
    for k in r['want']:
        outs[k] = Buf(dev, int(np.prod(shapes[k])), lead=r['dx_off'] if k == 'dx' else 0)
    optr = lambda k: outs[k].ptr if k in outs else None      # noqa: E731
    st = _lib.stream()
    tags = None
    try:
        if prof:
            _lib.check(lib.recnow_prof_enable(256), 'recnow_prof_enable')
            _lib.check(lib.recnow_prof_sample_every(1), 'recnow_prof_sample_every')
        _lib.call('recnow_multi_dense_fwd', x.ptr, xb, kernel.ptr, bias.ptr, B, D, U, N, act, outs['y'].ptr, ws.ptr, wb, st)
        torch.cuda.synchronize()
        fwd_tags = _gemm_tags(lib) if prof else None
        ws.nan()                  # the backward finds nothing of the forward in the workspace
        _lib.call('recnow_multi_dense_bwd', x.ptr, xb, kernel.ptr, outs['y'].ptr, dy.ptr, B, D, U, N, act, optr('dx'), optr('dkernel'),
                  optr('dbias'), ws.ptr, wb, st)
        torch.cuda.synchronize()
        if prof:
            tags = (fwd_tags, _gemm_tags(lib))
    finally:
        if prof:
            lib.recnow_prof_enable(0)
    for name, b in list(outs.items()) + [('workspace', ws), ('x', x), ('kernel', kernel), ('bias', bias), ('dy', dy)]:
        bad = b.damaged()
        assert bad == 0, '%s: %d sentinel words around %s changed' % (r['name'], bad, name)
    return {k: b.get(shapes[k]) for k, b in outs.items()}, tags


def _bits(a):
    """the fp32 words of a, with -0.0 as +0.0: they are the same number (a one-term product such as dz * 0 keeps the sign of its zero, a sum that
    starts from +0.0 does not; neither is a rounding)"""
    return (np.asarray(a, np.float32).reshape(-1) + np.float32(0.0)).view(np.int32)


def _row_margin(ref, got):
    """worst |err| / (REL max |ref| of the row) over the rows (last axis = the row's entries)"""
    err = np.abs(got.astype(np.float64) - ref).max(-1)
    return float((err / np.maximum(REL * np.abs(ref).max(-1), 1e-37)).max())


def _term_margin(ref, mag, got):
    """worst |err| / (REL sum of |terms| of the entry)"""
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(REL * mag, 1e-37)).max())


def check_empty(dev, r):
    inp = T.integer_inputs(r)
    got, tags = run(dev, r, inp, T.RELU, prof=True)
    assert tags == ([], [])
    assert got['y'].size == 0 and got['dx'].size == 0
    for k in ('dkernel', 'dbias'):
        assert (_bits(got[k]) == 0).all(), '%s: %s is not zeroed for an empty batch' % (r['name'], k)


def check_row(dev, r, idx):
    from _chunked_oracle import close
    if r['B'] == 0:
        return check_empty(dev, r)
    inp = T.integer_inputs(r)
    for act in (T.LINEAR, T.RELU):
        got, tags = run(dev, r, inp, act, prof=True)
        want, _ = T.reference(r, inp, act)
        assert set(got) == {'y'} | set(r['want'])
        for k in got:
            w, g = _bits(want[k]), _bits(got[k])
            bad = np.flatnonzero(w != g)
            assert bad.size == 0, '%s act %d integer %s: %d of %d words differ, first flat %d: %r vs %r' % (
                r['name'], act, k, bad.size, w.size, bad[0], got[k].reshape(-1)[bad[0]], want[k].reshape(-1)[bad[0]])
        assert (len(tags[0]), len(tags[1])) == (r['gemm_fwd'], r['gemm_bwd']), '%s act %d: GEMM tags %r forward / %r backward, expected %d / %d' % (
            r['name'], act, tags[0], tags[1], r['gemm_fwd'], r['gemm_bwd'])
    act = RANDOM_ACTS[idx % len(RANDOM_ACTS)]
    inp = T.random_inputs(r)
    got, _ = run(dev, r, inp, act)
    ref, mag = T.reference(r, inp, act)
    margins = {}
    for k in got:
        assert np.isfinite(got[k]).all(), '%s random: non-finite %s' % (r['name'], k)
        close(got[k], ref[k], what='%s random %s' % (r['name'], k))
        margins[k] = _row_margin(ref[k], got[k]) if k in ('y', 'dx') else _term_margin(ref[k], mag[k], got[k])
    worst = max(margins, key=margins.get)
    print('%s act %d: worst per-row / per-entry margin %.3f of the bound (%s)' % (r['name'], act, margins[worst], worst))
    over = {k: v for k, v in margins.items() if v > 1.0}
    assert not over, '%s random act %d: beyond the row / entry bound (fraction of it): %r' % (r['name'], act, over)


@pytest.mark.parametrize('ir', list(enumerate(T.ROUTES)), ids=[r['name'] for r in T.ROUTES])
def test_dense_route(dev, ir):
    check_row(dev, ir[1], ir[0])
