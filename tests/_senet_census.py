"""SENET (csrc/senet_fused.hip, the k_senet_* kernels of csrc/interact.hip) restated in numpy, for tests/test_senet_routes_gpu.py and
tests/test_senet_census_cpu.py.

  senet(.., dt=float64)        the closed form of the whole layer -- squeeze, two dense layers with any of the four activations, scale, every gradient --
                               with the cancellation-free magnitude of every sum next to it (scales=True): absolute values pushed through the same
                               graph, mean |x|, then |sq| |W1| + |b1| (+ |act(0)|: a sigmoid of 0 is 1/2), the next layer likewise, the activations'
                               Lipschitz constant of at most 1; backwards the same, and where a derivative is taken from a rounded output (1 - h^2,
                               w (1 - w)) the scale of what it multiplies carries that output's scale times the derivative's slope.  A scale of 0 demands
                               an error of 0.  The reference values of the GPU test come from oracle/dense_ref.senet_layer under fp64 autograd; this form
                               supplies the scales and is held to the oracle by the CPU test.  Sums go into a +0 accumulator (`+ 0.0`).
  entries(.., dt=float64)      the four unfused entries on their own inputs (w, dout and dsq are data there)
  .. (dt=float32, geom=..)     the same in fp32 in the factorisation of the row's kernels (tests/_senet_routes.py geometry()): the float4 partial sum
                               (x + y) + (z + w), the Q / 2 .. 1 butterfly, the P-way split of k with its butterfly, the sequential m loop, the weight
                               gradients per step of 4 rows, then per workgroup over its steps, then over the workgroups (rn_colsum is a tree of its
                               own, csrc/gemm.hip, with a census of its own: numpy's pairwise sum stands for it), the tile kernel's sequential column
                               sum.  Compilers contract a * b + c and the kernels' exp differs from numpy's by an ulp: neither changes a census bit, and
                               on random data both stay far inside the half bound the CPU test holds the restatement to.  `mistake` plants one error.
  make(r) / exact(r, c)        census data: integer inputs, weights and gradients without a zero among them, linear / relu activations (tanh -> linear,
                               sigmoid -> relu), magnitudes shrunk on LADDER until every scale -- every sum |terms| any kernel forms, the sums over B of the
                               weight gradients included -- stays below 2^24: fp32 in ANY order then gives the fp64 value to the bit.  Means and dsq / D_f
                               are exact: a field whose width is a power of two gives multiples of 1 / D (the bound counts in that unit), any other holds multiples of its width, and W1 (and the dsq handed to
                               recnow_senet_scale_bwd_x) multiples of the lcm of those widths.  Rows differ from row to row and fields from field to field.
  random_data(r)               N(0, 1) inputs and gradients, glorot-uniform weights, N(0, 0.05) biases; with relu every pre-activation is CLEAR x its
                               magnitude from 0 (rows are redrawn until they are; the callers assert KINK on the fp64 values)."""
import math
import zlib

import numpy as np

import _senet_routes as T
from _dcn_census import EXACT, REL, same_bits        # noqa: F401  (the project's conventions: 2^24, 1e-5, bit equality with zero signs)
from _rowop_census import KINK, _fold_halves, _seq        # noqa: F401

CLEAR = 1e-3          # what random_data() clears: ten times KINK (1e-4 of the pre-activation's magnitude, far above the (F + 2) 2^-24 of an fp32 dot product)
LADDER = [(3, 2, 2), (2, 2, 1), (2, 1, 1), (1, 1, 1)]           # (|x| in 1 .. xmax, |weight| in 1 .. wmax, |gradient| in 1 .. gmax)
MISTAKES = ('prefetch_not_advanced', 'rows_past_B_counted', 'half_butterfly', 'dsq_over_total', 'fwd8_last_pass_dropped', 'bias_grad_skipped',
            'tile_offset_shifted', 'act2_grad_from_h', 'last_slot_not_stored')
FUSED_OUT = ('out', 'sq', 'h', 'w', 'dx', 'dW1', 'db1', 'dW2', 'db2')
ENTRY_OUT = ('e_sq', 'e_out', 'e_dw', 'e_dx')


def act(z, code, dt):
    if code == T.RELU:
        return np.where(z > 0, z, dt(0))
    if code == T.TANH:
        return np.tanh(z).astype(dt)
    if code == T.SIGMOID:
        return (dt(1) / (dt(1) + np.exp(-z))).astype(dt)
    return z


def act_grad(y, code, dt):
    """the derivative from the OUTPUT y, as rn_act_grad_from_out"""
    if code == T.RELU:
        return np.where(y > 0, dt(1), dt(0))
    if code == T.TANH:
        return dt(1) - y * y
    if code == T.SIGMOID:
        return y * (dt(1) - y)
    return np.ones_like(y)


def _slope(y, code):
    """|d act'(y) / d y|: what an error of the output does to the derivative taken from it"""
    if code == T.TANH:
        return 2 * np.abs(y)
    if code == T.SIGMOID:
        return np.abs(1 - 2 * y)
    return np.zeros_like(y)


def _at0(code):
    return 0.5 if code == T.SIGMOID else 0.0


def _cols(dims):
    return np.repeat(np.arange(len(dims)), dims)


def census_acts(acts):
    return tuple({T.TANH: T.LINEAR, T.SIGMOID: T.RELU}.get(a, a) for a in acts)


# ---- the layer ------------------------------------------------------------------------------------------------------------------------------------------
def senet(d, acts, dt=np.float64, geom=None, mistake=None, scales=False):
    """d: x (list of (B, D_f)), W1 (F, M), b1 (M) or None, W2 (M, F), b2 (F) or None, dout (B, total).  Returns out, sq, h, w, dx (list), dW1, db1,
    dW2, db2, z1, z2 (the pre-activations); with scales s_* of each.  geom: geometry(row) of a fused row (None: the plain closed form)."""
    xs = [np.asarray(x, dt) for x in d['x']]
    dims = [x.shape[1] for x in xs]
    B, F = xs[0].shape[0], len(xs)
    W1, W2 = np.asarray(d['W1'], dt), np.asarray(d['W2'], dt)
    M = W1.shape[1]
    b1 = None if d.get('b1') is None else np.asarray(d['b1'], dt)
    b2 = None if d.get('b2') is None else np.asarray(d['b2'], dt)
    dout = np.asarray(d['dout'], dt)
    a1, a2 = acts
    col = _cols(dims)
    gf = geom['f'] if geom else None
    gb = geom['b'] if geom else None
    D = dims[0]
    X = np.stack(xs, 1) if geom else None                       # (B, F, D): fused rows have equal widths
    G = dout.reshape(B, F, D) if geom else None

    def lanes(v):                                                # (B, F, D) -> (B, F): float4 partial, then the butterfly over Q lanes
        Q = D // 4
        v4 = v.reshape(B, F, Q, 4)
        p = (v4[..., 0] + v4[..., 1]) + (v4[..., 2] + v4[..., 3])
        if mistake == 'half_butterfly' and Q >= 2:
            p = p[:, :, :Q // 2]                                 # the butterfly started at Q / 4: lane 0 hears from half the field's lanes
        return _fold_halves(p, 2)

    def split(a, Wt, P):                                         # sum_k a[b][k] Wt[k][m] with k dealt to P lanes, then the butterfly over them
        K = a.shape[1]
        parts = []
        for part in range(P):
            acc = np.zeros((B, Wt.shape[1]), dt)
            for k in range(part, K, P):
                acc = acc + a[:, k, None] * Wt[None, k, :]
            parts.append(acc)
        return _fold_halves(np.stack(parts, -1), 2)

    # forward
    Xf = X
    if gf is not None:
        src = np.arange(B)
        if mistake == 'prefetch_not_advanced' and B > gf['stride']:
            src[gf['stride']:] -= gf['stride']                   # request(b0) instead of request(nb0): the second pass computes on the first pass's rows
        Xf = X[src]
        if mistake == 'fwd8_last_pass_dropped' and gf['family'] == T.SF_FWD8:
            Xf = Xf.copy()
            Xf[:, F - 8:] = 0                                    # `p < NP - 1`: the fields 8 (NP - 1) .. F - 1 are never loaded
        sq = lanes(Xf) / dt(D)
        z1 = split(sq, W1, gf['P']) + (b1 if b1 is not None else dt(0))
        h = act(z1, a1, dt)
        z2 = np.zeros((B, F), dt) + (b2 if b2 is not None else dt(0))
        for m in range(M):
            z2 = z2 + h[:, m, None] * W2[None, m, :]
        w = act(z2, a2, dt)
        out = (Xf * w[:, :, None]).reshape(B, F * D)
    else:
        sq = np.stack([x.sum(1) + 0.0 for x in xs], 1) / np.asarray(dims, dt)
        z1 = (sq @ W1 + 0.0) + (b1 if b1 is not None else dt(0))
        h = act(z1, a1, dt)
        z2 = (h @ W2 + 0.0) + (b2 if b2 is not None else dt(0))
        w = act(z2, a2, dt)
        out = np.concatenate(xs, 1) * w[:, col]
    res = dict(out=out, sq=sq, h=h, w=w, z1=z1, z2=z2)
    # backward (the fused backward reads sq, h and w as the forward saved them)
    if gb is not None:
        src = np.arange(B)
        if mistake == 'prefetch_not_advanced' and B > gb['stride']:
            src[gb['stride']:] -= gb['stride']
        Xb, Gb = X[src], G[src]
        dw = lanes(Xb * Gb)
        # planted: `rn_act_grad_from_out(hs[..], dm.act2)` -- the hidden vector (unit k % M) where the excitation w belongs
        dz2 = dw * act_grad(h[:, np.arange(F) % M] if mistake == 'act2_grad_from_h' else w, a2, dt)
        dz1 = split(dz2, W2.T, gb['P']) * act_grad(h, a1, dt)
        dsq = np.zeros((B, F), dt)
        for m in range(M):
            dsq = dsq + dz1[:, m, None] * W1[None, :, m]
        div = dt(F * D) if mistake == 'dsq_over_total' else dt(D)
        dx = Gb * w[:, :, None] + (dsq / div)[:, :, None]
        res['dx'] = [np.ascontiguousarray(dx[:, f]) for f in range(F)]
        # weight gradients: per step of 4 rows from 0, per workgroup over its steps, then over the workgroups
        grid, stride = gb['grid'], gb['stride']
        npass = -(-B // stride)
        pad = npass * stride - B

        def byrow(a):                                            # (B, n) -> (passes, grid, 4, n), rows past B zero
            if mistake == 'rows_past_B_counted' and pad:
                tail = np.repeat(a[-1:], pad, 0)                 # the clamped rows of the last step are not masked: row B - 1 again and again
            else:
                tail = np.zeros((pad,) + a.shape[1:], dt)
            return np.concatenate([a, tail], 0).reshape(npass, grid, 4, -1)

        def wsum(a, b):                                          # sum_b a[b][i] b[b][j]
            pa, pb = byrow(a), byrow(b)
            acc = np.zeros((grid, a.shape[1], b.shape[1]), dt)
            for s in range(npass):
                step = np.zeros_like(acc)
                for j in range(4):
                    step = step + pa[s, :, j, :, None] * pb[s, :, j, None, :]
                acc = acc + step
            return acc.sum(0, dtype=dt) + dt(0)

        one = np.ones((B, 1), dt)
        dW1, dW2 = wsum(sq, dz1), wsum(h, dz2)
        db1, db2 = wsum(one, dz1)[0], wsum(one, dz2)[0]
        if mistake == 'bias_grad_skipped':
            db1 = np.zeros_like(db1)                             # the `o < 2 * FM + M` branch never taken: db1 stays the unused slot's 0
        if mistake == 'last_slot_not_stored':
            flat = np.concatenate([dW1.reshape(-1), dW2.reshape(-1), db1, db2])
            flat[256 * ((flat.size - 1) // 256):] = 0            # the store loop ran to NACC - 1 ... of the slots in use
            dW1, dW2 = flat[:F * M].reshape(F, M), flat[F * M:2 * F * M].reshape(M, F)
            db1, db2 = flat[2 * F * M:2 * F * M + M], flat[2 * F * M + M:]
    else:
        dwc = dout * np.concatenate(xs, 1)
        dw = np.stack([dwc[:, col == f].sum(1) + 0.0 for f in range(F)], 1)
        dz2 = dw * act_grad(w, a2, dt)
        dz1 = (dz2 @ W2.T + 0.0) * act_grad(h, a1, dt)
        dsq = dz1 @ W1.T + 0.0
        res['dx'] = [dout[:, col == f] * w[:, f, None] + (dsq[:, f] / dt(dims[f]))[:, None] for f in range(F)]
        dW1, dW2 = sq.T @ dz1 + 0.0, h.T @ dz2 + 0.0
        db1, db2 = dz1.sum(0) + 0.0, dz2.sum(0) + 0.0
    res.update(dW1=dW1, dW2=dW2, db1=db1, db2=db2)
    if scales:
        aW1, aW2 = np.abs(W1), np.abs(W2)
        s_sq = np.stack([np.abs(x).sum(1) for x in xs], 1) / np.asarray(dims, dt)
        s_z1 = s_sq @ aW1 + (np.abs(b1) if b1 is not None else 0)
        s_h = s_z1 + _at0(a1)
        s_z2 = s_h @ aW2 + (np.abs(b2) if b2 is not None else 0)
        s_w = s_z2 + _at0(a2)
        ax, ag = np.abs(np.concatenate(xs, 1)), np.abs(dout)
        s_dwc = ag * ax
        s_dw = np.stack([s_dwc[:, col == f].sum(1) for f in range(F)], 1)
        s_dz2 = s_dw * (np.abs(act_grad(w, a2, dt)) + _slope(w, a2) * s_w)
        s_dz1 = (s_dz2 @ aW2.T) * (np.abs(act_grad(h, a1, dt)) + _slope(h, a1) * s_h)
        s_dsq = s_dz1 @ aW1.T
        res.update(s_sq=s_sq, s_h=s_h, s_w=s_w, s_z1=s_z1, s_z2=s_z2, s_out=ax * s_w[:, col],
                   s_dx=[ag[:, col == f] * s_w[:, f, None] + (s_dsq[:, f] / dims[f])[:, None] for f in range(F)],
                   s_dW1=s_sq.T @ s_dz1, s_dW2=s_h.T @ s_dz2, s_db1=s_dz1.sum(0), s_db2=s_dz2.sum(0), s_dsq=s_dsq, s_dz1=s_dz1, s_dz2=s_dz2)
    return res


# ---- the four unfused entries -----------------------------------------------------------------------------------------------------------------------------
def entries(d, dt=np.float64, geom=None, mistake=None, scales=False):
    """d: x (list of (B, D_f)), w (B, F), dout (B, total), dsq (B, F).  Returns e_sq (B, F), e_out (B, total), e_dw (B, F), e_dx (list); with scales
    s_e_sq = mean |x|, s_e_out = |x| |w|, s_e_dw = sum |dout x|, s_e_dx = |dout| |w| + |dsq| / D_f."""
    xs = [np.asarray(x, dt) for x in d['x']]
    dims = [x.shape[1] for x in xs]
    B, F = xs[0].shape[0], len(xs)
    w, dout, dsq = np.asarray(d['w'], dt), np.asarray(d['dout'], dt), np.asarray(d['dsq'], dt)
    offs = np.concatenate([[0], np.cumsum(dims)[:-1]]).astype(int)
    total = sum(dims)
    e = geom['u'] if geom else None
    gs = [dout[:, o:o + n] for o, n in zip(offs, dims)]
    if e is not None and e['family'] == T.SENET_TILE and mistake == 'tile_offset_shifted':
        # `o = offs[f + 1]`: every field reads the tile columns of the next one (the last wraps to what lies there: column 0 on, taken as the row's start)
        sh = list(offs[1:]) + [0]
        gs = [np.take(dout, (o + np.arange(n)) % total, axis=1) for o, n in zip(sh, dims)]

    def rowsum(v, D):
        if e is None:
            return v.sum(1) + 0.0
        if e['family'] == T.SENET_TILE:
            return _seq(v, 1, dt)
        Q = D // 4
        v4 = v.reshape(B, Q, 4)
        p = (v4[..., 0] + v4[..., 1]) + (v4[..., 2] + v4[..., 3])
        if mistake == 'half_butterfly' and Q >= 2:
            p = p[:, :Q // 2]
        return _fold_halves(p, 1)

    xsrc = xs
    if e is not None and mistake == 'prefetch_not_advanced' and B > e['stride']:
        src = np.arange(B)
        src[e['stride']:] -= e['stride']                          # the second pass of the grid-stride loop works on the first pass's rows
        xsrc = [x[src] for x in xs]
    sq = np.stack([rowsum(x, n) / dt(n) for x, n in zip(xsrc, dims)], 1)
    out = np.concatenate([x * w[:, f, None] for f, x in enumerate(xsrc)], 1)
    dw = np.stack([rowsum(g * x, n) for g, x, n in zip(gs, xsrc, dims)], 1)
    div = [dt(total) if mistake == 'dsq_over_total' else dt(n) for n in dims]
    dx = [g * w[:, f, None] + (dsq[:, f] / div[f])[:, None] for f, g in enumerate(gs)]
    res = dict(e_sq=sq, e_out=out, e_dw=dw, e_dx=dx)
    if scales:
        ax, ag, aw = [np.abs(x) for x in xs], np.abs(dout), np.abs(w)
        ags = [ag[:, o:o + n] for o, n in zip(offs, dims)]
        res.update(s_e_sq=np.stack([a.sum(1) / n for a, n in zip(ax, dims)], 1), s_e_out=np.concatenate([a * aw[:, f, None] for f, a in enumerate(ax)], 1),
                   s_e_dw=np.stack([(g * a).sum(1) for g, a in zip(ags, ax)], 1),
                   s_e_dx=[g * aw[:, f, None] + (np.abs(dsq[:, f]) / n)[:, None] for f, (g, n) in enumerate(zip(ags, dims))])
    return res


# ---- one interface ------------------------------------------------------------------------------------------------------------------------------------------
def outputs(r, tag='C'):
    """what a run of row r returns: the C ABI of a fused row (tag 'C'), of an unfused row (the four entries), or the layer (tag 'layer')"""
    if tag == 'layer':
        return ('out', 'dx', 'dW1', 'dW2') + (('db1', 'db2') if r['b1'] else ())
    if r['kind'] == 'unfused':
        return ENTRY_OUT
    return tuple(k for k in FUSED_OUT if not (k == 'db1' and not r['b1']) and not (k == 'db2' and not r['b2']))


def model(r, d, acts=None, dt=np.float64, restate=False, mistake=None, scales=False, geom=None):
    g = (geom or T.geometry(r)) if (restate and r['kind'] == 'fused') else None
    return senet(d, acts or r['acts'], dt, g, mistake, scales)


def entry(r, d, dt=np.float64, restate=False, mistake=None, scales=False):
    return entries(d, dt, T.geometry(r) if restate else None, mistake, scales)


def compute(r, d, acts=None, dt=np.float64, restate=False, mistake=None, scales=False):
    """everything the C run of row r returns (fused: the layer's tensors; unfused: the four entries)"""
    return model(r, d, acts, dt, restate, mistake, scales) if r['kind'] == 'fused' else entry(r, d, dt, restate, mistake, scales)


def _flat(v):
    return np.concatenate([np.asarray(a, np.float64).reshape(len(a), -1) for a in v], 1) if isinstance(v, list) else np.asarray(v, np.float64)


def margins(keys, got, ref, sc, rel=REL):
    """worst |got - ref| / (rel x scale) per output, entry by entry against the entry's own scale; a scale of 0 demands an error of 0"""
    tiny = 1e-300
    m = {}
    for k in keys:
        a, e, s = _flat(got[k]), _flat(ref[k]), _flat(sc['s_' + k])
        assert a.shape == e.shape == s.shape, (k, a.shape, e.shape, s.shape)
        m[k] = float((np.abs(a - e) / np.maximum(rel * s, tiny)).max()) if e.size else 0.0
    return m


def bits_equal(a, b):
    return same_bits(_flat(a), _flat(b))


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------------------
def oracle(d, acts):
    """the layer on data d through oracle/dense_ref.senet_layer in fp64, gradients by autograd"""
    import torch
    import dense_ref as R
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double().requires_grad_(True)            # noqa: E731
    xs = [t64(x) for x in d['x']]
    k = [t64(d['W1']), t64(d['W2'])]
    bs = [None if d.get('b1') is None else t64(d['b1']), None if d.get('b2') is None else t64(d['b2'])]
    y = R.senet_layer(xs, k, bs, T.ACT_NAMES[acts[0]], T.ACT_NAMES[acts[1]])
    leaves = xs + k + [b for b in bs if b is not None]
    grads = torch.autograd.grad(y, leaves, torch.from_numpy(np.ascontiguousarray(d['dout'])).double(), allow_unused=True)
    F = len(xs)
    g = [None if v is None else v.numpy() for v in grads]
    res = dict(out=y.detach().numpy(), dx=g[:F], dW1=g[F], dW2=g[F + 1])
    rest = g[F + 2:]
    if bs[0] is not None:
        res['db1'] = rest.pop(0)
    if bs[1] is not None:
        res['db2'] = rest.pop(0)
    return res


# ---- data -----------------------------------------------------------------------------------------------------------------------------------------------
def _nonzero(rng, hi, shape):
    v = rng.integers(-hi, hi, shape, dtype=np.int8)               # -hi .. hi - 1, then the non-negative half moves up one: no zero
    v[v >= 0] += 1
    return v.astype(np.int32)


def _pow2(n):
    return n & (n - 1) == 0


def width_lcm(dims):
    return math.lcm(*([n for n in dims if not _pow2(n)] or [1]))


def _on(rng, r):
    B = r['B']
    if B <= 4096:
        return np.ones(B, bool)
    on = rng.random(B) < 1 / 16
    on[T.pinned_rows(r)] = True
    return on


def _draw(r, xmax, wmax, gmax):
    rng = np.random.default_rng(zlib.crc32(('senet census ' + r['name']).encode()))
    B, dims, M = r['B'], r['dims'], r['M']
    F = len(dims)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)                      # noqa: E731
    lcm = width_lcm(dims)
    on = _on(rng, r)
    d = dict(x=[f32(_nonzero(rng, xmax, (B, n)) * (1 if _pow2(n) else n)) for n in dims], dout=f32(_nonzero(rng, gmax, (B, sum(dims))) * on[:, None]))
    if r['kind'] == 'unfused':
        d.update(w=f32(_nonzero(rng, wmax, (B, F))), dsq=f32(_nonzero(rng, gmax, (B, F)) * lcm))
    if not r['census_only']:
        d.update(W1=f32(_nonzero(rng, wmax, (F, M)) * lcm), W2=f32(_nonzero(rng, wmax, (M, F))),
                 b1=f32(_nonzero(rng, wmax, M)) if r['b1'] else None, b2=f32(_nonzero(rng, wmax, F)) if r['b2'] else None)
    return d


def denominator(dims):
    """the means over a power-of-two width D are multiples of 1 / D, and so is everything computed from them: the largest such D"""
    return max([n for n in dims if _pow2(n)] or [1])


def largest_sum(r, d):
    """the largest sum |terms| over every sum a kernel of row r forms on d, in units of 1 / denominator(dims) -- every term is a multiple of that
    unit, so a sum whose magnitudes stay below 2^24 units is exact in fp32 in any order"""
    big, unit = [], denominator(r['dims'])
    if not r['census_only'] and r.get('layer_census', True):
        e = model(r, d, census_acts(r['acts']), scales=True)
        big += [unit * float(np.max(_flat(v))) for k, v in e.items() if k.startswith('s_') and np.size(_flat(v))]
    if r['kind'] == 'unfused':
        # the entries on their own inputs: the row sums of integers (before the division by D_f) and dout w are integers; dsq / D_f alone is not
        e = entry(r, d, scales=True)
        big += [float(max(np.abs(x).sum(1).max() for x in d['x'])), float(e['s_e_dw'].max()), float(e['s_e_out'].max()), unit * float(np.max(_flat(e['s_e_dx'])))]
    return max(big)


_MADE = {}


def make(r, params=None):
    """the census of route row r: the first LADDER entry on which every sum is exact (params: that entry, already known).  Returns (data, entry)."""
    if params is None and r['name'] in _MADE:
        return _MADE[r['name']]
    for p in ([params] if params else LADDER):
        d = _draw(r, *p)
        if params or r['census_only'] or largest_sum(r, d) < EXACT:
            if params is None:
                _MADE[r['name']] = (d, p)
            return d, p
    raise AssertionError('no census parameters keep %s exact' % r['name'])


def _near_kink(d, acts):
    """rows with a relu pre-activation within CLEAR of its magnitude of 0"""
    e = senet(d, acts, scales=True)
    bad = np.zeros(len(e['z1']), bool)
    if acts[0] == T.RELU:
        bad |= (np.abs(e['z1']) < CLEAR * e['s_z1']).any(1)
    if acts[1] == T.RELU:
        bad |= (np.abs(e['z2']) < CLEAR * e['s_z2']).any(1)
    return bad


def kink_clearance(d, acts):
    """smallest |z| / scale over the relu pre-activations in fp64 (inf without relu)"""
    e = senet(d, acts, scales=True)
    lo = np.inf
    if acts[0] == T.RELU:
        lo = min(lo, float((np.abs(e['z1']) / e['s_z1']).min()))
    if acts[1] == T.RELU:
        lo = min(lo, float((np.abs(e['z2']) / e['s_z2']).min()))
    return lo


def random_data(r):
    """x and the gradients ~ N(0, 1), W glorot-uniform as the layer's initialiser, biases N(0, 0.05).  Nothing here cancels beyond what the scales
    account for: every output entry's scale is the sum of the magnitudes of its own terms.  relu: the rows with a pre-activation within CLEAR x its
    magnitude of 0 are drawn again until none is left -- a sign flip at the kink is fp32's doing, not a kernel's."""
    rng = np.random.default_rng(zlib.crc32(('senet random ' + r['name']).encode()))
    B, dims, M = r['B'], r['dims'], r['M']
    F = len(dims)
    n32 = lambda *s: rng.normal(0, 1, s).astype(np.float32)                  # noqa: E731
    lim = math.sqrt(6.0 / (F + M))
    d = dict(x=[n32(B, n) for n in dims], dout=n32(B, sum(dims)), W1=rng.uniform(-lim, lim, (F, M)).astype(np.float32),
             W2=rng.uniform(-lim, lim, (M, F)).astype(np.float32), b1=(0.05 * n32(M)) if r['b1'] else None, b2=(0.05 * n32(F)) if r['b2'] else None)
    if r['kind'] == 'unfused':
        d.update(w=n32(B, F), dsq=n32(B, F))
    if T.RELU in r['acts']:
        for _ in range(400):
            bad = np.flatnonzero(_near_kink(d, r['acts']))
            if not bad.size:
                break
            for x in d['x']:
                x[bad] = n32(bad.size, x.shape[1])
        else:
            raise AssertionError('%s: rows stay within CLEAR of a relu kink' % r['name'])
    return d
