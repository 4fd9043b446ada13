"""Every exact-fp32 GEMM route, bit for bit on integer census data, inside guard bands (tests/_gemm_routes.py, tests/_exact_census.py).

One row per k_gemm instantiation of csrc/gemm_inst_*.hip and per split-K reduce / XCD remap form.  Each row runs in precision 0 and checks:
  1. census bits: C (and Cx, as_out) equal the exact census element for element, with LINEAR and RELU epilogues;
  2. guard bands: every operand sits in a NaN-filled buffer (>= 4 floats of leading-dimension padding, 256 rows of NaN before and after, a NaN row
     between batches), so a read outside a logical matrix would change the census result; C, Cx and as_out sit in sentinel buffers laid out the
     same way, and the workspace has a sentinel tail past recnow_gemm_workspace_bytes: every sentinel word must survive bit for bit;
  3. planted non-finite values: a NaN and an inf in A and in B make exactly the outputs whose fp64 reference is non-finite non-finite; every other
     output is bit-identical to the clean census run;
  4. random data: |C - R|_ij <= C_ELEM (|A'||B'|)_ij plus the ulps of the epilogue terms, side product included, and the norm bound of
     test_gemm_fuzz;
  5. route and tile family: recnow_gemm_route names the row's kernel (tests/_gemm_routes.py check_route) for the very descriptor and workspace size
     being launched, and the launch's recnow_prof tag is the row's family (never the short-K kernel's);
  6. TANH / SIGMOID epilogues on the census pre-activations stay within rn_act's documented error, and every route maps the same pre-activation to
     the same bits (test_act_routes_agree).
Left out: XF 25, the fused sub-space forward (tests/test_midf_gpu.py reaches it through the layer oracle); the split-precision and the short-K
kernels (tests/test_split_routes_gpu.py covers them in both arithmetics).  test_act_sweep runs about 4 M inputs of rn_act through an edge route
(K = 1) and a lean route (K = 32, one nonzero k per output)."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import _exact_census as E
import _gemm_routes as R
from _gemm_routes import ROUTES, TAG_SHORTK

pytestmark = pytest.mark.gpu

# per-element bound on random data, |C - R|_ij <= C_ELEM (|A'||B'|)_ij: a host emulation of the k-ordered fp32 fma chain (one rounding per
# term, U(-1, 1) operands, 128 x 128 outputs) gave at most 2.3e-7 at K = 384, 2.0e-7 at K = 1024, 1.9e-7 at K = 8192 (the longest chain of the
# table: the K >= 16384 rule's slabs of 8192; slabs are summed in fp64); the operand modes add at most 3 roundings of A' (1.8e-7 relative):
# 1e-6 is 2.4x their sum
C_ELEM = 1e-6
U = 2.0 ** -23                    # one rounding of an epilogue term, with a factor 2 of margin
SENT = 0x7FC0DEAD                 # sentinel word of the output buffers (a NaN no kernel computes)
TANH_ABS = 1.5e-7                 # rn_tanh for |x| >= 0.25 (csrc/common.hpp: "about 2e-7 absolute"; test_act_sweep measured 1.27e-7)
ACT_REL = 2.0 ** -21              # rn_tanh's odd series below 0.25 and rn_act's SIGMOID 1 / (1 + expf(-x)): 4 ulp relative
TINY = 2.0 ** -126                # sigmoid below -87.3 (subnormal results, expf overflow at -88.7): absolute

ACT_SEEN = {}                     # (act, z bits) -> (output bits, route): the activated census outputs of every route


class Buf:
    """The matrix of a Geo (tests/_gemm_routes.py) inside its guard-banded flat device buffer, filled with `fill` around the stored `data`."""

    def __init__(self, dev, geo, fill=float('nan'), data=None):
        g = self.geo = geo
        self.buf = torch.full((g.words,), fill, dtype=torch.float32, device=dev)
        self.view = self.buf[g.pre:g.pre + g.nb * g.sb].view(g.nb, g.rows + 1, g.ld)[:, :g.rows, :g.cols]
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data)).to(dev).repeat(1, g.rep[0], g.rep[1]))

    def intact(self):
        """every word outside the logical matrix still holds the sentinel"""
        g = self.geo
        bits = self.buf.view(torch.int32)
        outside = torch.ones_like(bits, dtype=torch.bool)
        outside[g.pre:g.pre + g.nb * g.sb].view(g.nb, -1, g.ld)[:, :g.rows, :g.cols] = False
        return int(((bits != SENT) & outside).sum())

    def get(self):
        return self.view.cpu().numpy()


def _sent_float():
    return float(np.array([SENT], np.uint32).view(np.float32)[0])


def run(dev, spec, extra, st, act=E.LINEAR, prof=False, route=None):
    """One recnow_gemm of `spec` on the stored operands `st` (census or random; arrays of the census's shapes).  Returns (C (batch, M, N),
    Cx, as_out, tags) and checks every sentinel.  route = (name, kernel): recnow_gemm_route names the row's kernel for the very descriptor and
    workspace size of the launch."""
    from rec_now_amd import _lib
    lib = _lib.load()
    s = spec
    M, N = s['M'], s['N']
    perm = extra.get('perm', 0)
    shapes = {k: st[k].shape for k in ('A', 'A2', 'B', 'B2') if k in st}
    assert shapes == R.stored_shapes(R.census_spec(spec, extra)[1])
    geo = R.geometry(s, extra, shapes)
    sent = _sent_float()
    data = {'A': st['A'], 'A2': st.get('A2'), 'B': st['B'], 'B2': st.get('B2'), 'bias': st.get('bias'), 'E': st.get('E'), 'Bx': st.get('Bx'),
            'P': st.get('P'), 'Q': st.get('Q'), 'as_in': st.get('as_in')}
    if s['accumulate']:
        data['C'] = st['C0'].transpose(0, 2, 1) if s['c_trans'] else st['C0']
    outputs = ('C', 'Cx', 'as_out')
    bufs = {k: Buf(dev, g, fill=sent if k in outputs else float('nan'), data=data.get(k)) for k, g in geo.items()}
    d = R.fill_desc(_lib.GemmDesc(), s, extra, act, geo, {k: b.buf.data_ptr() for k, b in bufs.items()})
    c, cx, aso = bufs['C'], bufs.get('Cx'), bufs.get('as_out')
    outs = [bufs[k] for k in outputs if k in bufs]
    wsb = int(lib.recnow_gemm_workspace_bytes(ctypes.byref(d)))
    ws = torch.full((wsb // 4 + 4096,), sent, dtype=torch.float32, device=dev)
    tags = None
    if prof:
        _lib.check(lib.recnow_prof_enable(16), 'recnow_prof_enable')
        _lib.check(lib.recnow_prof_sample_every(1), 'recnow_prof_sample_every')
    if route is not None:
        info = _lib.GemmRouteInfo()
        assert lib.recnow_gemm_route(ctypes.byref(d), wsb, ctypes.byref(info)) == 0, '%s: recnow_gemm_route refuses the descriptor' % route[0]
        R.check_route(route[0], route[1], extra, info)
    try:
        _lib.call('recnow_gemm', ctypes.byref(d), ctypes.c_void_p(ws.data_ptr()), wsb, _lib.stream())
        torch.cuda.synchronize()
        if prof:
            cap = 16
            t, t0, t1 = (ctypes.c_int * cap)(), (ctypes.c_double * cap)(), (ctypes.c_double * cap)()
            n = lib.recnow_prof_intervals(t, t0, t1, cap)
            tags = [t[i] for i in range(max(n, 0))]
    finally:
        if prof:
            lib.recnow_prof_enable(0)
    for o, what in zip(outs, [k for k in outputs if k in bufs]):
        bad = o.intact()
        assert bad == 0, '%d sentinel words of %s changed (leading-dimension padding, rows before / after, batch gaps)' % (bad, what)
    tail = ws[wsb // 4:].view(torch.int32)
    assert bool((tail == SENT).all()), 'workspace written past recnow_gemm_workspace_bytes = %d' % wsb
    C = c.get()
    if perm:
        C = C.reshape(N // perm, M, perm).transpose(1, 0, 2).reshape(1, M, N)
    elif s['c_trans']:
        C = C.transpose(0, 2, 1)
    return C, (cx.get()[0] if cx else None), (aso.get()[0] if aso else None), tags


def _tiled(x, extra):
    mt, nt = extra.get('tile', (1, 1))
    return np.tile(x, (1, mt, nt)) if (mt, nt) != (1, 1) else x


def _same(tag, got, want):
    wrong = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert wrong.size == 0, '%s: %d of %d outputs differ from the census, first flat %d: %r vs %r' % (
        tag, wrong.size, want.size, wrong[0], got.reshape(-1)[wrong[0]], want.reshape(-1)[wrong[0]])


def _act_err(ref, act):
    """documented error of rn_act at the fp64 value ref"""
    if act == E.TANH:
        return np.where(np.abs(ref) >= np.tanh(0.25), TANH_ABS, ACT_REL * np.abs(ref) + TINY)
    if act == E.SIGMOID:
        return ACT_REL * np.abs(ref) + TINY
    return np.zeros_like(ref)


def _bound(c, z, act, den):
    """per-element error bound of the epilogue: the product's den = C_ELEM |A'||B'| (+ rank-R terms), carried through bias, act, emul, C0."""
    s = c.spec
    e = den + U * np.abs(z)
    y = E.apply_act(c, z, act)
    lip = {E.LINEAR: 1.0, E.RELU: 1.0, E.TANH: 1.0, E.SIGMOID: 0.25}[act]
    cols = s['act_cols'] or s['N']
    e[..., :cols] = lip * e[..., :cols] + _act_err(y[..., :cols], act)
    if s['e_mode']:
        Ef = c.stored['E'].astype(np.float64)
        Ef = Ef if s['e_mode'] == E.MUL else E.act_grad(Ef, s['e_act'])
        e = e * np.abs(Ef) + 3 * U * np.abs(y * Ef)
        y = y * Ef
    if s['accumulate']:
        y = y + c.stored['C0']
        e = e + U * (np.abs(y) + np.abs(c.stored['C0']))
    return y, e


def _random_stored(c, rng):
    st = {}
    for k, v in c.stored.items():
        if k in ('A2', 'B2') and c.spec[('a' if k == 'A2' else 'b') + '_mode'] == E.ACTGRAD:
            act = c.spec['a_act' if k == 'A2' else 'b_act']
            st[k] = (rng.uniform(0.05, 0.95, v.shape) if act == E.SIGMOID else rng.uniform(-0.95, 0.95, v.shape)).astype(np.float32)
        elif k == 'E' and c.spec['e_mode'] == E.ACTGRAD:
            st[k] = (rng.uniform(0.05, 0.95, v.shape) if c.spec['e_act'] == E.SIGMOID else rng.uniform(-0.95, 0.95, v.shape)).astype(np.float32)
        else:
            st[k] = np.where(v == 0, 0.0, rng.uniform(-1, 1, v.shape)).astype(np.float32)      # (keeps the k_valid zero padding)
    return st


def _with(c, st):
    r = E.Census()
    r.spec, r.stored = c.spec, st
    r.Ae, r.Be = E.effective(c.spec, st, 'A'), E.effective(c.spec, st, 'B')
    return r


def check_row(dev, name, kern, spec, extra):
    from rec_now_amd import _lib
    full, cs = R.census_spec(spec, extra)
    c = E.make(cs)
    staging = extra.get('staging')
    if staging is not None:
        _lib.call('recnow_set_gemm_staging', staging)
    try:
        clean = None
        for act in (E.LINEAR, E.RELU):
            C, Cx, aso, tags = run(dev, full, extra, c.stored, act, prof=(act == E.LINEAR), route=(name, kern))
            if tags is not None:
                assert tags and TAG_SHORTK not in tags and set(tags) == {extra['tag']}, '%s: launch tags %r, expected %d' % (name, tags, extra['tag'])
            want, wx, wa = E.expected(c, act)
            _same('%s census act %d C' % (name, act), C, _tiled(want, extra))
            if wx is not None:
                _same('%s census act %d Cx' % (name, act), Cx, wx)
            if wa is not None:
                _same('%s census as_out' % name, aso, wa)
            if act == E.LINEAR:
                clean = (C, Cx, aso)
        # TANH / SIGMOID on the exact pre-activations
        z = E.preactivation(c)
        for act in (E.TANH, E.SIGMOID):
            C, _, _, _ = run(dev, full, extra, c.stored, act)
            C = C[:, :cs['M'], :cs['N']]
            ref, err = _bound(c, z, act, 0 * z)
            bad = ~(np.abs(C - ref) <= err)
            assert not bad.any(), '%s act %d: %d outputs beyond the documented error, worst %.3g' % (name, act, int(bad.sum()), np.abs(C - ref)[bad].max())
            if not full['e_mode'] and not full['accumulate']:
                cols = full['act_cols'] or cs['N']
                zb = z[..., :cols].astype(np.float32).view(np.int32).reshape(-1)
                ob = C[..., :cols].view(np.int32).reshape(-1)
                for zz, oo in zip(*np.unique(np.stack([zb, ob], 1), axis=0).T):
                    prev = ACT_SEEN.setdefault((act, int(zz)), (int(oo), name))
                    if prev[0] != int(oo):
                        ACT_SEEN.setdefault('conflicts', []).append((act, int(zz), prev, (int(oo), name)))
        # planted non-finite values (LINEAR: RELU maps NaN to 0)
        if extra.get('tile', (1, 1)) == (1, 1):
            rng = np.random.default_rng(zlib.crc32(name.encode()))
            st = {k: v.copy() for k, v in c.stored.items()}
            for side, vals in (('A', (np.nan, np.inf)), ('B', (-np.inf, np.nan))):
                sh = st[side].shape
                for v in vals:
                    st[side][0, rng.integers(sh[1]), rng.integers(sh[2])] = v
            p = _with(c, st)
            C, Cx, aso, _ = run(dev, full, extra, st)
            with np.errstate(invalid='ignore'):
                rowbad = ~np.isfinite(p.Ae).all(2)                    # (batch, M)
                colbad = ~np.isfinite(p.Be).all(1)                    # (batch, N)
            bad = rowbad[:, :, None] | colbad[:, None, :]
            assert bad.any()
            assert not np.isfinite(C[bad]).any(), '%s: %d outputs with a non-finite reference are finite' % (name, int(np.isfinite(C[bad]).sum()))
            assert np.array_equal(C[~bad].view(np.int32), clean[0][~bad].view(np.int32)), '%s: %d finite outputs moved' % (
                name, int((C[~bad] != clean[0][~bad]).sum()))
            if Cx is not None:
                assert not np.isfinite(Cx[rowbad[0]]).any() and np.array_equal(Cx[~rowbad[0]], clean[1][~rowbad[0]]), '%s: side product' % name
            if aso is not None:
                nf = ~np.isfinite(st['A'][0])
                assert not np.isfinite(aso[nf]).any() and np.array_equal(aso[~nf], clean[2][~nf]), '%s: as_out' % name
        # random data, per element
        rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
        r = _with(c, _random_stored(c, rng))
        C, Cx, aso, _ = run(dev, full, extra, r.stored)
        C = C[:, :cs['M'], :cs['N']]
        z = E.preactivation(r)
        den = C_ELEM * (np.abs(r.Ae) @ np.abs(r.Be))
        if cs['eu_r']:
            den = den + U * (np.abs(r.stored['P'][0].astype(np.float64)) @ np.abs(r.stored['Q'][0].astype(np.float64)))
        ref, err = _bound(r, z, E.LINEAR, den)
        assert np.isfinite(C).all(), '%s random: non-finite output' % name
        assert np.abs(C - ref).max() <= 3e-7 * (np.abs(r.Ae) @ np.abs(r.Be)).max() + 2e-6, '%s random: norm bound' % name
        over = np.abs(C - ref) > err
        assert not over.any(), '%s random: %d outputs beyond the per-element bound, worst err %.3g' % (name, int(over.sum()), np.abs(C - ref)[over].max())
        if Cx is not None:
            Rx = r.Ae[0] @ r.stored['Bx'][0].astype(np.float64)
            dx = C_ELEM * (np.abs(r.Ae[0]) @ np.abs(r.stored['Bx'][0].astype(np.float64)))
            assert (np.abs(Cx - Rx) <= dx).all(), '%s random: side product beyond C_ELEM' % name
        if aso is not None:
            assert np.array_equal(aso, r.stored['A'][0] * r.stored['as_in'][0]), '%s random: as_out' % name
    finally:
        if staging is not None:
            _lib.call('recnow_set_gemm_staging', 0)


@pytest.mark.parametrize('route', ROUTES, ids=[r[0] for r in ROUTES])
def test_gemm_route(dev, route):
    name, kern, spec, extra, _ = route
    from rec_now_amd import _lib
    _lib.call('recnow_set_gemm_precision', 0)
    check_row(dev, name, kern, spec, extra)


def test_split_precision_refusal_is_tagged_fp32(dev):
    """Precision 1 with a side product over TWO column tiles (M 128, N 256, K 512, interior, aligned): the split kernels take one column tile only,
    so the plan names the fp32 k_gemm of the 128 x 128 family (two-wide side product, XF 9), the launch is tagged with that family and not with
    RN_TAG_GEMM_SPLIT, and the output is the precision-0 run's bit for bit."""
    from rec_now_amd import _lib
    spec, extra = dict(M=128, N=256, K=512, sp_r=2), {'tag': R.T128, 'reduce': 1}
    kern = R.kname(128, 128, 32, True, False, False, 0, 0, 9)
    full, cs = R.census_spec(spec, extra)
    c = E.make(cs)
    got = {}
    try:
        for prec in (1, 0):
            _lib.call('recnow_set_gemm_precision', prec)
            C, Cx, _, tags = run(dev, full, extra, c.stored, prof=True, route=('two column tiles, precision %d' % prec, kern))
            assert tags == [R.T128], 'precision %d: launch tags %r' % (prec, tags)
            got[prec] = (C, Cx)
    finally:
        _lib.call('recnow_set_gemm_precision', 0)
    assert np.array_equal(got[1][0].view(np.int32), got[0][0].view(np.int32)) and np.array_equal(got[1][1].view(np.int32), got[0][1].view(np.int32))
    want, wx, _ = E.expected(c, E.LINEAR)
    _same('two column tiles C', got[1][0], want)
    _same('two column tiles Cx', got[1][1], wx)


def test_act_routes_agree(dev):
    """Every route maps one exact pre-activation to one activated output (TANH, SIGMOID; rows without emul / accumulate)."""
    routes = {v[1] for k, v in ACT_SEEN.items() if k != 'conflicts'}
    if len(routes) < 2:
        pytest.skip('needs the route rows of this module first')
    assert not ACT_SEEN.get('conflicts'), ACT_SEEN['conflicts'][:10]


def _sweep_inputs():
    f32 = np.float32
    tiny = np.array([0.0, -0.0, 1e-45, 1e-40, 1e-39, 1.1754942e-38, 1.1754944e-38, 1.2e-38, 1e-30, 1e-20, 1e-10, 1e-5], f32)
    near = []
    for x in (0.25, 1e-3, 88.0, 89.0, 88.72283, 87.33654):
        v = np.float32(x)
        for _ in range(8):
            v = np.nextafter(v, np.float32(np.inf))
            near.append(v)
        v = np.float32(x)
        near.append(v)
        for _ in range(8):
            v = np.nextafter(v, np.float32(-np.inf))
            near.append(v)
    near = np.array(near, f32)
    dense = np.linspace(-20, 20, 3 << 20, dtype=np.float64).astype(f32)
    small = np.geomspace(1e-7, 0.5, 1 << 18).astype(f32)
    x = np.concatenate([tiny, -tiny, near, -near, dense, small, -small, np.geomspace(20, 100, 4096).astype(f32)])
    x = x[np.isfinite(x)]
    pad = (-x.size) % 4096
    return np.concatenate([x, np.zeros(pad, f32)])


def _gemm_plain(dev, A, B, act):
    from rec_now_amd import _lib
    lib = _lib.load()
    M, K = A.shape
    N = B.shape[1]
    Ad, Bd = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    C = torch.empty((M, N), device=dev)
    d = _lib.GemmDesc()
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc = Ad.data_ptr(), K, Bd.data_ptr(), N, C.data_ptr(), N
    d.M, d.N, d.K, d.batch, d.act = M, N, K, 1, act
    ws = _lib.workspace(lib.recnow_gemm_workspace_bytes(ctypes.byref(d)), dev)
    _lib.call('recnow_gemm', ctypes.byref(d), _lib.ptr(ws), ws.numel(), _lib.stream())
    torch.cuda.synchronize()
    return C.cpu().numpy()


@pytest.mark.parametrize('act', [E.TANH, E.SIGMOID], ids=['tanh', 'sigmoid'])
def test_act_sweep(dev, act):
    """rn_act over ~4 M inputs through an edge route (K = 1, N = 1: 256 x 32 family) and a lean route (K = 32, N = 128, one nonzero k per output:
    lean 128 x 128 BK 16), bitwise against each other and within the documented error of fp64; +-inf and NaN through the edge route."""
    from rec_now_amd import _lib
    _lib.call('recnow_set_gemm_precision', 0)
    x = _sweep_inputs()
    edge = _gemm_plain(dev, x[:, None], np.ones((1, 1), np.float32), act)[:, 0]
    B = (np.arange(32)[:, None] == np.arange(128)[None, :] % 32).astype(np.float32)
    lean = _gemm_plain(dev, x.reshape(-1, 32), B, act)
    lean = lean[:, :32].reshape(-1)
    assert np.array_equal(lean.view(np.int32), edge.view(np.int32)), 'edge and lean routes differ on %d inputs, e.g. x = %r' % (
        int((lean != edge).sum()), x[np.flatnonzero(lean != edge)[:4]])
    ref = E.act64(x.astype(np.float64), act)
    err = np.abs(edge - ref)
    lim = _act_err(ref, act)
    big = np.abs(x) >= 0.25
    print('act %d: max abs err |x| >= 0.25: %.3g; max rel err below: %.3g' % (act, err[big].max(), (err[~big] / np.maximum(np.abs(ref[~big]), 1e-38)).max()))
    assert (err <= lim).all(), 'act %d: %d inputs beyond the documented error, worst at x = %r (err %.3g)' % (
        act, int((err > lim).sum()), x[np.argmax(err - lim)], err.max())
    special = np.array([np.inf, -np.inf, np.nan, 0.0], np.float32)
    got = _gemm_plain(dev, special[:, None], np.ones((1, 1), np.float32), act)[:, 0]
    want = np.array([1.0, -1.0] if act == E.TANH else [1.0, 0.0], np.float32)
    assert np.array_equal(got[:2], want) and np.isnan(got[2]) and got[3] == E.act64(np.zeros(1), act)[0], got
