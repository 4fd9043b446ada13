"""DCN-v1 (csrc/dcn.hip) restated in numpy, three ways, for tests/test_dcn_routes_gpu.py and tests/test_dcn_census_cpu.py:

  cross(.., dt=float64)   the closed form the kernels use -- per row the scalars c_l = x_l . w_l, x_{l+1} = act(x0 c_l + b_l); backward dz_l = g_l act'(out_l),
                          dc_l = <dz_l, x0>, dx0 = sum_l dz_l c_l + dc_0 w_0, g_{l-1} = dc_l w_l, dW_l = sum_rows x_l dc_l, db_l = sum_rows dz_l -- with the
                          cancellation-free magnitude of every sum next to it.  The reference values of the GPU test come from oracle/dense_ref.dcn_layer
                          under fp64 autograd; this form supplies the scales (and is held to the autograd oracle by the CPU test).
  cross(.., dt=float32, geom=..)
                          the same in fp32 in the kernels' factorisation: a row's dot as per-lane partial sums over the lane's (nv x vec) elements, then a
                          butterfly over the lanes (and over the waves of a row); weight gradients per (workgroup, row slot) over the passes of the
                          grid-stride loop, over the row slots of a workgroup, then over the workgroup slabs (numpy's pairwise sum stands in for the
                          column sum).  `mistake` plants one error (MISTAKES).
  make(row) / exact(c)    census data: integer inputs on which every sum any kernel forms -- over d, over the layers into dx0, over the rows into dW and db
                          -- keeps sum |terms| < 2^24, so fp32 in ANY order gives the fp64 value to the bit.  linear and relu (relu keeps integers
                          integer; its derivative is taken from the output, 0 at 0, as torch's)."""
import zlib

import numpy as np

LINEAR, RELU, TANH, SIGMOID = 0, 1, 2, 3
ACT_ORACLE = {LINEAR: None, RELU: 'relu', TANH: 'tanh', SIGMOID: 'sigmoid'}
EXACT = float(1 << 24)
# (k nonzero entries of +-1 per kernel row, |x0| in 1 .. xmax, density of the hashed dy rows): shrunk until every sum is exact
LADDER = [(3, 2, 1 / 16), (2, 2, 1 / 32), (2, 2, 1 / 128), (2, 1, 1 / 128), (1, 1, 1 / 256), (1, 1, 0.0)]
MISTAKES = ('drop_last_row_second_pass', 'prefetch_clamp', 'xl_wrong_layer_c', 'xl_wrong_layer_b', 'dx0_without_g', 'db_before_act_grad', 'slab_left_out',
            'waves_not_combined')


def act_np(z, act):
    if act == RELU:
        return np.where(z > 0, z, z.dtype.type(0))
    if act == TANH:
        return np.tanh(z)
    if act == SIGMOID:
        return (1 / (1 + np.exp(-z))).astype(z.dtype)
    return z


def act_grad_from_out(y, act):
    if act == RELU:
        return (y > 0).astype(y.dtype)
    if act == TANH:
        return 1 - y * y
    if act == SIGMOID:
        return y * (1 - y)
    return np.ones_like(y)


def geometry(cfg, B, grid_cap=2048):
    """rows per workgroup and workgroups of a (tpr, vec, nv) kernel (csrc/dcn.hip dcn_grid; grid_cap: the occupancy cap of the fast backward)"""
    tpr = cfg[0] or 256
    rpb = 256 // tpr
    return dict(tpr=tpr, vec=cfg[1] or 1, rpb=rpb, G=max(1, min((B + rpb - 1) // rpb, 2048, grid_cap)))


def _lane_dot(prod, geom, wave_only=False):
    """sum over the last axis of prod (B, D) in fp32 as the kernels form it: element d = (i tpr + t) vec + e belongs to lane t; a lane adds its elements
    in order, then the lanes are added pairwise (butterfly).  wave_only: every element gets the sum of ITS wave only (planted mistake)."""
    Bn, D = prod.shape
    tpr, vec = geom['tpr'], geom['vec']
    nv = -(-D // (tpr * vec))
    pad = np.zeros((Bn, nv * tpr * vec), prod.dtype)
    pad[:, :D] = prod
    lanes = pad.reshape(Bn, nv, tpr, vec).transpose(0, 2, 1, 3).reshape(Bn, tpr, nv * vec)
    if wave_only:
        # TPR = 128: lanes t and t + 64 sit in different waves and are never added
        assert tpr == 128
        per_elem = np.zeros((Bn, nv, tpr, vec), prod.dtype)
        per_elem[:, :, :64] = lanes[:, :64].sum((1, 2), dtype=prod.dtype)[:, None, None, None]
        per_elem[:, :, 64:] = lanes[:, 64:].sum((1, 2), dtype=prod.dtype)[:, None, None, None]
        return per_elem.reshape(Bn, -1)[:, :D]
    acc = np.zeros((Bn, tpr), prod.dtype)
    for j in range(nv * vec):
        acc = acc + lanes[:, :, j]
    while acc.shape[1] > 1:
        h = acc.shape[1] // 2
        acc = acc[:, :h] + acc[:, h:]             # (which lanes pair up does not matter to the census; to the error estimate hardly)
    return acc[:, 0]


def _col_sum(rows, geom, skip_wg=None):
    """sum over the rows of (B, D) as the kernels form it: per (workgroup, row slot) over the passes, over the row slots, over the workgroups"""
    Bn, D = rows.shape
    G, rpb = geom['G'], geom['rpb']
    P = -(-Bn // (G * rpb))
    pad = np.zeros((P * G * rpb, D), rows.dtype)
    pad[:Bn] = rows
    pad = pad.reshape(P, G, rpb, D)
    acc = np.zeros((G, rpb, D), rows.dtype)
    for p in range(P):
        acc = acc + pad[p]
    slab = np.zeros((G, D), rows.dtype)
    for r in range(rpb):
        slab = slab + acc[:, r]
    if skip_wg is not None:
        slab[skip_wg] = 0
    return slab.sum(0, dtype=rows.dtype)


def cross(x, w, b, dy, act, dt=np.float64, geom=None, bgeom=None, mistake=None, scales=False):
    """forward and backward of the cross stack.  x, dy (B, D); w (L, D); b (L, D) or None.  geom / bgeom: the forward / backward kernel geometry
    (None: plain numpy sums).  Returns y, c (B, L), dx, dW, db (L, D); with scales the cancellation-free magnitudes s_y, s_dx (B), s_c, s_dc (B, L), s_dW,
    s_db (L, D) (see tests/test_dcn_routes_gpu.py)."""
    x, dy, w = np.asarray(x, dt), np.asarray(dy, dt), np.asarray(w, dt)
    Bn, D = x.shape
    L = w.shape[0]
    bz = np.zeros((L, D), dt) if b is None else np.asarray(b, dt)
    dot = (lambda p, g, **k: p.sum(1, dtype=dt)) if geom is None else _lane_dot
    col = (lambda r, g, **k: r.sum(0, dtype=dt)) if bgeom is None else _col_sum
    xs = x
    if mistake == 'prefetch_clamp' and geom is not None:
        # the two arms of the next-row clamp swapped: where a next pass exists the request re-reads the own row (pass p then computes on the rows of
        # pass p - 1); on the last pass it reads row + stride past B, which nothing consumes
        stride = geom['G'] * geom['rpb']
        src = np.arange(Bn)
        src[stride:] -= stride
        xs = x[src]
    c = np.zeros((Bn, L), dt)
    s_c = np.zeros((Bn, L), dt)
    t_run = np.zeros(Bn, dt)
    xl = xs
    for l in range(L):
        c[:, l] = dot(xl * w[l], geom)
        if scales:
            s_c[:, l] = np.maximum(s_c[:, l - 1] if l else 0, np.abs(xl * w[l]).sum(1))
            t_run = np.maximum(t_run, np.abs(xs).max(1) * np.abs(xl * w[l]).sum(1) + np.abs(bz[l]).max())
        xl = act_np(xs * c[:, l:l + 1] + bz[l], act)
    y = xl
    res = dict(y=y, c=c)
    # backward (the saved-scalars factorisation of dcn_bwd_saved_body / k_dcn_bwd_fast; the recompute and general kernels form the same values)
    g = dy.copy()
    gm = np.abs(dy)
    dx = np.zeros((Bn, D), dt)
    dxm = np.zeros((Bn, D), dt)
    dW, db = np.zeros((L, D), dt), np.zeros((L, D), dt)
    s_dW, s_db, s_dc = np.zeros((L, D), dt), np.zeros((L, D), dt), np.zeros((Bn, L), dt)
    wave_only = mistake == 'waves_not_combined'
    skip = 0 if mistake == 'slab_left_out' else None
    for l in range(L - 1, -1, -1):
        cl = c[:, l:l + 1]
        out = act_np(xs * cl + bz[l], act)
        if mistake == 'db_before_act_grad':
            db[l] = col(g, bgeom, skip_wg=skip)
        ga = act_grad_from_out(out, act)
        g = g * ga
        gm = gm * np.abs(ga)
        dc = dot(g * xs, bgeom or geom, **({'wave_only': True} if wave_only else {}))
        dc = dc if wave_only else dc[:, None]
        pm = (gm * np.abs(xs)).sum(1)[:, None]
        lc, lb = (l, l) if mistake == 'xl_wrong_layer_c' else (l - 1, l - 1)
        if mistake == 'xl_wrong_layer_b':
            lb = l
        xlv = xs if l == 0 else act_np(xs * c[:, lc:lc + 1] + bz[lb], act)
        if mistake != 'db_before_act_grad':
            db[l] = col(g, bgeom, skip_wg=skip)
        dx = dx + g * cl
        dW[l] = col(xlv * dc, bgeom, skip_wg=skip)
        if scales:
            s_db[l] = np.abs(g).sum(0)
            s_dc[:, l] = pm[:, 0]
            s_dW[l] = np.abs(xlv * dc).sum(0)
            dxm = dxm + gm * np.abs(cl)
        g = dc * w[l]
        gm = pm * np.abs(w[l])
    if mistake != 'dx0_without_g':
        dx = dx + g
    if mistake == 'drop_last_row_second_pass' and geom is not None:
        # workgroup 0 leaves the last row of its second pass out: y and dx of that row are not written, its weight-gradient terms are missing
        r = geom['G'] * geom['rpb'] + geom['rpb'] - 1
        assert r < Bn
        one = cross(x[r:r + 1], w, b, dy[r:r + 1], act, dt)
        y = y.copy()
        y[r], dx[r] = 0, 0
        dW, db = dW - one['dW'], db - one['db']
        res['y'] = y
    res.update(dx=dx, dW=dW, db=db)
    if scales:
        res.update(s_y=t_run, s_c=s_c, s_dx=(dxm + gm).max(1), s_dc=s_dc, s_dW=s_dW, s_db=s_db)
    return res


# ---- census ---------------------------------------------------------------------------------------------------------------------------------
class Census:
    pass


def pinned_rows(B):
    """rows that always carry dy: the first and the last row, and every row of workgroup 0 in every pass, for every grid the kernels can run a batch
    of B rows on (1, 2 or 4 rows per workgroup; 2048 workgroups, or 256 x occupancy 1 .. 8 in the fast backward)"""
    rows = {0, B - 1}
    for rpb in (1, 2, 4):
        for G in {min((B + rpb - 1) // rpb, cap) for cap in [2048] + [256 * o for o in range(1, 9)]}:
            for r0 in range(0, B, G * rpb):
                rows |= {r for r in range(r0, min(B, r0 + rpb))}
    return np.array(sorted(rows))


def _draw(r, k, xmax, rho, act):
    rng = np.random.default_rng(zlib.crc32(('dcn census ' + r['name']).encode()))
    B, D, L = r['B'], r['D'], r['L']
    c = Census()
    c.act, c.params = act, (k, xmax, rho)
    c.x = (rng.integers(1, xmax + 1, (B, D)) * rng.choice([-1, 1], (B, D))).astype(np.float32)
    c.w = np.zeros((L, D), np.float32)
    for l in range(L):
        pos = rng.choice(D, min(k, D), replace=False)
        c.w[l, pos] = rng.choice([-1, 1], pos.size)
    c.b = rng.integers(-2, 3, (L, D)).astype(np.float32) if r['bias'] else None
    on = rng.random(B) < rho
    on[pinned_rows(B)] = True
    c.dy = (rng.choice([-1, 1], (B, D)) * on[:, None]).astype(np.float32)
    return c


def sums_exact(c):
    """the largest sum |terms| over every sum the kernels form on this census (all of them must stay below 2^24)"""
    e = cross(c.x, c.w, c.b, c.dy, c.act, scales=True)
    # s_y is max|x0| sum|x_l w_l| + max|b|: above every |x0 c| + |b|; s_dx: the backward on magnitudes, above every partial sum into dx0
    return max(float(e[k].max()) for k in ('s_y', 's_c', 's_dx', 's_dc', 's_dW', 's_db'))


def make(r, act=LINEAR, params=None):
    """the census of route row r: the first LADDER entry on which every sum is exact (params: that entry, already known)"""
    for p in ([params] if params else LADDER):
        c = _draw(r, *p, act)
        if params or sums_exact(c) < EXACT:
            return c
    raise AssertionError('no census parameters keep %s exact' % r['name'])


def exact(c):
    """y, c, dx, dW, db of the census in fp64 (every value an integer below 2^24: exact, and exactly representable in fp32)"""
    return cross(c.x, c.w, c.b, c.dy, c.act)


def same_bits(a, b):
    """a and b (taken to fp32) agree bit for bit, the sign of a zero included"""
    a, b = np.ascontiguousarray(a, np.float32).reshape(-1), np.ascontiguousarray(np.asarray(b).astype(np.float32)).reshape(-1)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


# ---- random data for the fp64 comparison ----------------------------------------------------------------------------------------------------------
KINK = 1e-3                       # the distance from a kink every pre-activation of a relu row must keep in the fp64 oracle (asserted by the caller)
CLEAR = 0.02                      # what random_data() clears: an element x_l,d = x0 c + b that nearly cancels carries its rounding (2^-24 of |x0 c| + |b|) into
                                  # dW_{l}, whose column scale under relu can be that one element


def random_data(r):
    """x = N(0, 1) + mu_row, dy = N(0, 1) + nu_row (mu, nu = +-U(0.5, 1.5) per row), w_l = (+-0.75 + U(-1, 1)) / D, b ~ U(-0.5, 0.5).  The offsets keep
    every row's c_l = x_l . w_l and dc_l = <dz_l, x0> away from 0 -- within a small factor of sum |terms| -- and |w| ~ 1 / D keeps c_l of order 1, so tanh
    and sigmoid do not saturate: with centred data c_l and dc_l are sqrt(D)-fold cancellations whose fp32 rounding, carried into dW_l = sum_rows x_l dc_l,
    is a property of the data and not of a kernel.  relu: elements whose pre-activation comes within CLEAR of 0 in fp64 are moved away (x0 pushed
    outwards) until none is left -- a sign flip at a kink is a property of fp32 too; the caller asserts the distance KINK on the fp64 oracle."""
    rng = np.random.default_rng(zlib.crc32(('dcn random ' + r['name']).encode()))
    B, D, L = r['B'], r['D'], r['L']
    off = lambda n: rng.uniform(0.5, 1.5, (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))      # noqa: E731
    x = (rng.normal(0, 1, (B, D)) + off(B)).astype(np.float32)
    w = ((rng.uniform(-1, 1, (L, D)) + 0.75 * rng.choice([-1.0, 1.0], (L, 1))) / D).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, (L, D)).astype(np.float32) if r.get('bias', True) else None
    dy = (rng.normal(0, 1, (B, D)) + off(B)).astype(np.float32)
    if r['act'] == RELU:
        for _ in range(200):
            near = min_preact(x, w, b, r['act'])[1]
            if not near.any():
                break
            x[near] += np.float32(0.25) * np.where(x[near] >= 0, 1, -1).astype(np.float32)
    return x, w, b, dy


def min_preact(x, w, b, act):
    """(smallest |pre-activation| over all layers in fp64, mask of the x0 elements within CLEAR of a kink)"""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    xl, lo, near = x64, np.inf, np.zeros(x64.shape, bool)
    for l in range(w64.shape[0]):
        z = x64 * (xl * w64[l]).sum(1, keepdims=True) + (0 if b is None else np.asarray(b[l], np.float64))
        lo = min(lo, float(np.abs(z).min()))
        near |= np.abs(z) < CLEAR
        xl = act_np(z, act)
    return lo, near


# ---- the bound of the fp64 comparison ---------------------------------------------------------------------------------------------------------
REL = 1e-5                        # the project's north-star tolerance (tests/test_layers_gpu.py RTOL)


def cfg_of(code):
    """(tpr, vec, nv) of a route code (tests/_dcn_routes.py code())"""
    return (code // 100 % 1000, code // 10 % 10, code % 10)


def margins(got, ref, sc, rel=REL):
    """worst |got - ref| / (rel x scale) per output: y and dx per row (the row's largest error against the row's scale), c per entry, dW and db per
    layer and column.  The scale is the cancellation-free magnitude of what was summed, in fp64 (cross(.., scales=True)):
      y     max_l (max_d |x0_d| sum_d |x_l,d w_l,d| + max_d |b_l,d|)            the largest magnitude a layer of this row summed, carried to the output
      c_l   max_{m <= l} sum_d |x_m,d w_m,d|
      dx    max_d of the backward on magnitudes: |dz_l| from |g_l|, sum_d |dz_l,d x0_d| for dc_l, sum_l |dz_l,d| |c_l| + that magnitude of dc_0 times |w_0,d|
      dW_l  sum_rows |x_l,d dc_l|          db_l  sum_rows |dz_l,d|
    A scale of 0 (nothing summed) demands an error of 0."""
    tiny = 1e-300
    f = lambda a: np.asarray(a, np.float64)                                  # noqa: E731
    m = {'y': float((np.abs(f(got['y']) - ref['y']).max(1) / np.maximum(rel * sc['s_y'], tiny)).max()),
         'dx': float((np.abs(f(got['dx']) - ref['dx']).max(1) / np.maximum(rel * sc['s_dx'], tiny)).max()),
         'dW': float((np.abs(f(got['dW']) - ref['dW']) / np.maximum(rel * sc['s_dW'], tiny)).max())}
    if got.get('c') is not None:
        m['c'] = float((np.abs(f(got['c']) - ref['c']) / np.maximum(rel * sc['s_c'], tiny)).max())
    if got.get('db') is not None:
        m['db'] = float((np.abs(f(got['db']) - ref['db']) / np.maximum(rel * sc['s_db'], tiny)).max())
    return m


def restate32(r, x, w, b, dy, mistake=None, grid_cap=2048):
    """fp32 in the factorisation of the kernels row r runs on"""
    return cross(x, w, b, dy, r['act'], np.float32, geometry(cfg_of(r['fwd']), r['B']), geometry(cfg_of(r['bwd']), r['B'], grid_cap), mistake)
