"""Every DCN-v2 layer route (tests/_mix_routes.py), bit for bit on integer census data (tests/_mix_census.py), inside guard bands, with its
kernels proven by their recnow_prof tags, and per row against fp64 on random data.

Per row, through the C ABI (recnow_dcn_mix_fwd/bwd, recnow_dcn_mix_score_fwd/bwd):
  1. census bits: LINEAR and RELU census data give every output and every gradient bit for bit;
  2. guard bands: `saved` and the workspace are NaN before the forward, the workspace NaN again before the backward (a read of a word nobody
     wrote poisons a census output); `saved`, the workspace and every output (y / scores, dx, each weight gradient, the head's gradients) have a
     sentinel tail past their declared size, and every output is NaN before the call: every sentinel word must survive, every output be written;
  3. route proof: with recnow_prof_enable / recnow_prof_sample_every(1), the route tags of the launches (RN_TAG_MIX_MID_FWD/BWD, GEMM_SPLIT,
     GEMM_MIDF, MIX_TILE_FWD/BWD) are exactly the row's, and recnow_dcn_mix_tile_route agrees (a route without a tag of its own -- the gate
     kernels -- is proven by the absence of the others);
  4. random data: TANH / SIGMOID activations, rows of x scaled by 2^-k (k in 0..8): per row of y and dx |err| <= 1e-5 max |ref| of the row, per
     expert slice and column of the weight gradients likewise (dW: 4e-5, see REL_DW), each score within 1e-5 of its row's sum of |y_d w_d|,
     and the norm bound of the layer tests (_chunked_oracle.close); the worst margin of every row is printed.
Rows with per-process switches (RECNOW_MIDF, RECNOW_XLESS) run in a child process per setting, one after another."""
import ctypes
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, 'oracle')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _mix_census as M                      # noqa: E402
from _mix_routes import ROUTES, ROUTE_TAGS, PROC_ENVS, spec      # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 0x7FC0DEAD                  # sentinel word (a NaN no kernel computes)
TAIL = 1024                        # sentinel words past every buffer
REL = 1e-5                         # per-row / per-column bound on random data
# dW per expert slice and column: plain fp32 arithmetic of the same formulas (tests/_mix_census.py restate in fp32, numpy products over the
# batch in order) already reaches 1.36 / 1.59 / 1.41 / 1.05 x REL of the column max on the random data of tile_d1024_l3 / split_l3 /
# score_mid_l4 / score_mid_l2: a column of dW = (x g)^T T2g sums B terms of one sign of T2g (SIGMOID: H2 > 0, G > 0) against random signs of
# x g, and inherits the relative error of g after up to three backward layers.  The kernels measured 1.02 - 1.44 x REL there.
REL_DW = 4e-5
PAIRS = ((M.TANH, M.TANH), (M.RELU, M.SIGMOID), (M.LINEAR, M.TANH), (M.SIGMOID, M.TANH), (M.TANH, M.SIGMOID))


class Buf:
    """n fp32 words (NaN) followed by TAIL sentinel words"""

    def __init__(self, dev, n, data=None):
        import torch
        self.n = int(n)
        self.buf = torch.full((self.n + TAIL,), float('nan'), dtype=torch.float32, device=dev)
        self.buf[self.n:].view(torch.int32).fill_(np.int32(np.uint32(SENT).view(np.int32)))
        if data is not None:
            self.buf[:self.n].copy_(torch.from_numpy(np.ascontiguousarray(data, np.float32).reshape(-1)).to(dev))
        self.ptr = self.buf.data_ptr()

    def nan(self):
        self.buf[:self.n].fill_(float('nan'))

    def intact(self):
        import torch
        return int((self.buf[self.n:].view(torch.int32) != np.int32(np.uint32(SENT).view(np.int32))).sum())

    def get(self, shape):
        return self.buf[:self.n].cpu().numpy().reshape(shape)


def _arr(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def run(dev, r, inp, ai, ao, prof=False):
    """One forward and backward of row r on inputs `inp` (census layout, float32).  Returns (outputs, tags, tile_route) and checks every sentinel."""
    import torch
    from rec_now_amd import _lib
    lib = _lib.load()
    B, D, S, N, L = r['B'], r['D'], r['S'], r['N'], r['L']
    head = r['entry'] == 'score'
    x = Buf(dev, B * D, inp['x'])
    Ws = {k: [Buf(dev, a.size, a) for a in inp[k]] for k in ('U', 'V', 'W', 'b', 'K')}
    P = {k: _arr([b.ptr for b in v]) for k, v in Ws.items()}
    sb = int(lib.recnow_dcn_mix_saved_bytes(B, D, S, N, L))
    wb = int(lib.recnow_dcn_mix_workspace_bytes(B, D, S, N, L))
    saved, ws = Buf(dev, sb // 4), Buf(dev, wb // 4)
    st = _lib.stream()
    st2 = _lib.side_stream(dev) if r['stream2'] else None
    shapes = {}
    outs = {}
    if head:
        hw, hb = Buf(dev, D, inp['hw']), Buf(dev, 1, inp['hb'])
        ds = Buf(dev, B, inp['ds'])
        outs['scores'] = Buf(dev, B)
        shapes['scores'] = (B,)
    else:
        dy = Buf(dev, B * D, inp['dy'])
        outs['y'] = Buf(dev, B * D)
        shapes['y'] = (B, D)
    if r['need_dx']:
        outs['dx'] = Buf(dev, B * D)
        shapes['dx'] = (B, D)
    g = {}
    for l in range(L):
        for k, shp in (('dU', (N, D, S)), ('dV', (N, S, S)), ('dW', (N, S, D)), ('db', (N, D)), ('dK', (D, N))):
            g.setdefault(k, []).append(Buf(dev, int(np.prod(shp))))
            outs['%s%d' % (k, l)] = g[k][-1]
            shapes['%s%d' % (k, l)] = shp
    G = {k: _arr([b.ptr for b in v]) for k, v in g.items()}
    if head:
        outs['dhead_w'], outs['dhead_b'] = Buf(dev, D), Buf(dev, 1)
        shapes['dhead_w'], shapes['dhead_b'] = (D,), (1,)
    saved_env = {k: os.environ.get(k) for k in r['call_env']}
    os.environ.update(r['call_env'])
    tags = None
    try:
        _lib.call('recnow_set_gemm_precision', r['prec'])
        route = int(lib.recnow_dcn_mix_tile_route(B, D, S, N, L))
        if prof:
            _lib.check(lib.recnow_prof_enable(4096), 'recnow_prof_enable')
            _lib.check(lib.recnow_prof_sample_every(1), 'recnow_prof_sample_every')
        if head:
            _lib.call('recnow_dcn_mix_score_fwd', x.ptr, P['U'], P['V'], P['W'], P['b'], P['K'], hw.ptr, hb.ptr, B, D, S, N, L, ai, ao,
                      outs['scores'].ptr, saved.ptr, sb, ws.ptr, wb, st, r['need_dx'])
        else:
            _lib.call('recnow_dcn_mix_fwd', x.ptr, P['U'], P['V'], P['W'], P['b'], P['K'], B, D, S, N, L, ai, ao, outs['y'].ptr, saved.ptr, sb,
                      ws.ptr, wb, st, r['need_dx'])
        torch.cuda.synchronize()
        ws.nan()                  # the backward finds nothing of the forward in the workspace
        _lib.call('recnow_set_gemm_precision', r['bprec'])
        dxp = outs['dx'].ptr if r['need_dx'] else None
        if head:
            _lib.call('recnow_dcn_mix_score_bwd', x.ptr, P['U'], P['V'], P['W'], P['b'], P['K'], hw.ptr, ds.ptr, saved.ptr, sb, B, D, S, N, L,
                      ai, ao, dxp, G['dU'], G['dV'], G['dW'], G['db'], G['dK'], outs['dhead_w'].ptr, outs['dhead_b'].ptr, ws.ptr, wb, st, st2,
                      None)
        else:
            _lib.call('recnow_dcn_mix_bwd', x.ptr, P['U'], P['V'], P['W'], P['b'], P['K'], dy.ptr, saved.ptr, sb, B, D, S, N, L, ai, ao, dxp,
                      G['dU'], G['dV'], G['dW'], G['db'], G['dK'], ws.ptr, wb, st, st2)
        torch.cuda.synchronize()
        if prof:
            cap = 4096
            t, t0, t1 = (ctypes.c_int * cap)(), (ctypes.c_double * cap)(), (ctypes.c_double * cap)()
            n = lib.recnow_prof_intervals(t, t0, t1, cap)
            assert 0 < n < cap, n
            tags = {t[i] for i in range(n)}
    finally:
        if prof:
            lib.recnow_prof_enable(0)
        _lib.call('recnow_set_gemm_precision', 0)
        for k, v in saved_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for name, b in list(outs.items()) + [('saved', saved), ('workspace', ws)]:
        bad = b.intact()
        assert bad == 0, '%s: %d sentinel words past %s changed' % (r['name'], bad, name)
    return {k: b.get(shapes[k]) for k, b in outs.items()}, tags, route


def _bits(a):
    return np.asarray(a, np.float32).reshape(-1).view(np.int32)


def _census_inputs(c):
    inp = dict(c.inp)
    inp['W'] = [w for w in c.inp['W']]
    return inp


def _random(r, seed):
    """random inputs of the row: weights at the layer tests' scales, rows of x scaled by 2^-k, k in 0..8"""
    rng = np.random.default_rng(seed)
    B, D, S, N, L = r['B'], r['D'], r['S'], r['N'], r['L']
    f = lambda *shape: rng.standard_normal(shape)      # noqa: E731
    k = rng.integers(0, 9, B)
    inp = {'x': (rng.uniform(-1, 1, (B, D)) * np.exp2(-k)[:, None])}
    inp['U'] = [f(N, D, S) / np.sqrt(D) for _ in range(L)]
    inp['V'] = [f(N, S, S) / np.sqrt(S) for _ in range(L)]
    inp['W'] = [f(N, S, D) / np.sqrt(S) for _ in range(L)]
    inp['b'] = [0.1 * f(N, D) for _ in range(L)]
    inp['K'] = [f(D, N) / np.sqrt(D) for _ in range(L)]
    if r['entry'] == 'score':
        inp['ds'] = rng.uniform(-1, 1, B)
        inp['hw'] = f(D) / np.sqrt(D)
        inp['hb'] = np.array([0.25])
    else:
        inp['dy'] = rng.uniform(-1, 1, (B, D))
    return {kk: ([a.astype(np.float32) for a in v] if isinstance(v, list) else v.astype(np.float32)) for kk, v in inp.items()}


def _cols(ref, got, axis_sets):
    """worst |err| / (REL max |ref|) over the slices that keep the axes in `axis_sets` (reduced over the others)"""
    err = np.abs(got.astype(np.float64) - ref)
    red = tuple(i for i in range(ref.ndim) if i not in axis_sets)
    scale = np.abs(ref).max(axis=red, keepdims=True) if red else np.abs(ref)
    return float((err / np.maximum(REL * scale, 1e-37)).max())


def check_row(dev, r, idx):
    from _chunked_oracle import close
    s = spec(r)
    c = M.make(**s, params=r['census'], verify=False)
    inp = _census_inputs(c)
    for ai, ao in ((M.LINEAR, M.LINEAR), (M.RELU, M.RELU)):
        got, tags, route = run(dev, r, inp, ai, ao, prof=(ai == M.LINEAR))
        want = M.expected(c, ai, ao)
        assert set(got) == set(k for k in want if not k.startswith('_'))
        for k in got:
            w, gk = _bits(want[k]), _bits(got[k])
            bad = np.flatnonzero(w != gk)
            assert bad.size == 0, '%s act %d/%d census %s: %d of %d words differ, first flat %d: %r vs %r' % (
                r['name'], ai, ao, k, bad.size, w.size, bad[0], got[k].reshape(-1)[bad[0]], want[k].reshape(-1)[bad[0]])
        if tags is not None:
            assert tags & ROUTE_TAGS == r['tags'], '%s: route tags %r, expected %r' % (r['name'], sorted(tags & ROUTE_TAGS), sorted(r['tags']))
        assert route == r['tile_route'], '%s: recnow_dcn_mix_tile_route %d, expected %d' % (r['name'], route, r['tile_route'])
    # random data, per row
    ai, ao = PAIRS[idx % len(PAIRS)]
    inp = _random(r, zlib.crc32(r['name'].encode()))
    got, _, _ = run(dev, r, inp, ai, ao)
    rc = M.Census()
    rc.spec, rc.inp = s, {k: ([a.astype(np.float64) for a in v] if isinstance(v, list) else v.astype(np.float64)) for k, v in inp.items()}
    ref = M.restate(rc, ai, ao, keep=True)
    margins = {}
    for k in got:
        assert np.isfinite(got[k]).all(), '%s random: non-finite %s' % (r['name'], k)
        close(got[k], ref[k], what='%s random %s' % (r['name'], k),
              scale=(np.abs(rc.inp['ds']).sum() if k == 'dhead_b' else None))
        if k in ('y', 'dx'):
            margins[k] = _cols(ref[k], got[k], (0,))                  # per row
        elif k == 'scores':
            # one number per row: its scale is the row's sum of |terms| y_d w_d (a relative bound on a sum that may cancel is no bound)
            y = ref['_keep']['x'][-1]
            sc = np.abs(y * rc.inp['hw'][None, :]).sum(1) + abs(rc.inp['hb'][0])
            margins[k] = float((np.abs(got[k] - ref[k]) / (REL * sc)).max())
        elif k[:2] in ('dU', 'dV'):
            margins[k] = _cols(ref[k], got[k], (0, 2))                # per expert slice n and column
        elif k[:2] == 'dW':
            margins[k] = _cols(ref[k], got[k], (0, 2)) * REL / REL_DW
        elif k[:2] == 'db':
            margins[k] = _cols(ref[k], got[k], (0,))                  # per expert slice
        elif k[:2] == 'dK':
            margins[k] = _cols(ref[k], got[k], (1,))                  # per gate column
    worst = max(margins, key=margins.get)
    print('%s act %d/%d: worst per-row / per-column margin %.3f of the bound (%s)' % (r['name'], ai, ao, margins[worst], worst))
    over = {k: v for k, v in margins.items() if v > 1.0}
    assert not over, '%s random act %d/%d: beyond the row / column bound (fraction of it): %r' % (r['name'], ai, ao, over)


_LOCAL = [(i, r) for i, r in enumerate(ROUTES) if not r['proc_env']]


@pytest.mark.parametrize('ir', _LOCAL, ids=[r['name'] for _, r in _LOCAL])
def test_mix_route(dev, ir):
    check_row(dev, ir[1], ir[0])


@pytest.mark.parametrize('penv', PROC_ENVS, ids=['-'.join('%s=%s' % kv for kv in p) for p in PROC_ENVS])
def test_mix_route_per_process_switch(dev, penv):
    """the rows that need a per-process switch, in a child process with it"""
    env = dict(os.environ, **dict(penv))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(dict(penv))], capture_output=True, text=True, timeout=600,
                         cwd=ROOT, env=env)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'rows passed' in out.stdout


if __name__ == '__main__':          # child: the rows of one per-process setting
    import torch
    want = json.loads(sys.argv[1])
    dev = torch.device('cuda:0')
    n = 0
    for i, r in enumerate(ROUTES):
        if r['proc_env'] == want:
            check_row(dev, r, i)
            n += 1
    assert n > 0
    print('%d rows passed' % n)
